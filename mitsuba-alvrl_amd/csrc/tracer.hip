// tracer.hip -- vrlTracer::randomWalk (vrlTracer.h:13-230) on the GPU,
// SURVEY.md 8(f) row 2.  One lane per particle: particle p draws from its own
// counter-based stream (seed, pass, p).  The walk, the eye-path chains and the
// records are transport.h's, the same source the host tracer
// (csrc/host/scene.cpp) compiles, so the VRL set, the records and the chains
// are the host's bit for bit -- diffuse, mirror, null and dielectric surfaces
// alike.  Built with -ffp-contract=off and IEEE division / square root like
// the host.  What is the device's own: the occluder query (the BVH instead of
// the host's loop over the triangles), where VRLs and records are written,
// and the capped per-lane stack of the chain walk.
//
// Two passes per batch of particles: count each particle's VRLs, then (after
// a prefix sum on the host picks the particles the sequential loop would have
// traced -- it stops after the particle that brings the set to the target)
// write them at their final positions in the SoA planes.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "alvrl_host.h"
#include "bvh_device.hpp"
#include "host/bvh.hpp"
#include "host/scene.hpp"
#include "transport.h"

namespace alvrl {
namespace host {
extern thread_local std::string g_host_err;
SmokeBox to_box(const alvrl_scene_desc& s);   // host_capi.cpp
const char* scene_problem(const alvrl_scene_desc& s);
}
}  // namespace alvrl

namespace {

using namespace alvrl;
using namespace alvrl::transport;

// The scene as the shared walks read it (the SceneView's pointers are device
// memory), with the occluder query of the device: the host-built BVH, whose
// closest hit takes the smallest t, ties to the lowest triangle index -- what
// the host's loop in index order finds.
struct TScene : SceneView {
    bvh::View bv;   // ntri == 0: none
    __device__ const float* closest_occluder(V3 o, V3 d, float mint, float* best, int* id, float* bu, float* bv_) const
    {
        int slot = 0;
        bvh::closest(bv, o, d, mint, best, id, &slot, bu, bv_);
        return bv.tris + 9 * (size_t)slot;
    }
};

// Sink's store: counts the accepted VRLs, and writes them into the SoA planes
// at 'pos' when soa != nullptr
struct PlaneStore {
    uint32_t n;
    float* soa;
    uint64_t pos, stride;
    __device__ void add(V3 start, V3 end, const float power[3])
    {
        if (soa) {
            const uint64_t i = pos + n;
            const float v[9] = {start.x, start.y, start.z, end.x, end.y, end.z, power[0], power[1], power[2]};
#pragma unroll
            for (int pl = 0; pl < 9; pl++) soa[(uint64_t)pl * stride + i] = v[pl];
        }
        n++;
    }
};

struct TArgs {
    uint32_t seed, pass;
    int short_vrls, max_depth, rr_depth;
};

// particle p's VRLs: counted (soa == nullptr), or written from position pos on
__device__ uint32_t trace(const TScene& sc, const TArgs& a, uint64_t p, float* soa, uint64_t pos, uint64_t stride)
{
    Stream smp(a.seed, a.pass, kDomTracer, (uint32_t)p, (uint32_t)(p >> 32));
    Sink<PlaneStore> k{};
    k.sigma_s_zero = !sc.medium.scatters();
    k.store.soa = soa;
    k.store.pos = pos;
    k.store.stride = stride;
    trace_particle(sc, smp, a.short_vrls != 0, a.max_depth, a.rr_depth, k);
    return k.store.n;
}

__global__ void __launch_bounds__(256) k_trace_count(TScene sc, TArgs a, uint64_t p0, uint32_t P, uint32_t* counts)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= P) return;
    counts[i] = trace(sc, a, p0 + i, nullptr, 0, 0);
}

__global__ void __launch_bounds__(256) k_trace_write(TScene sc, TArgs a, uint64_t p0, uint32_t P,
                                                     const uint64_t* offs, float* soa, uint64_t stride)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= P) return;
    (void)trace(sc, a, p0 + i, soa, offs[i], stride);
}

int terr(int code, const std::string& m)
{
    alvrl::host::g_host_err = m;
    return code;
}

template <typename T>
struct DMem {
    T* p = nullptr;
    ~DMem() { if (p) (void)hipFree(p); }
    hipError_t alloc(size_t n) { return hipMalloc(&p, std::max<size_t>(n, 1) * sizeof(T)); }
};

// The scene's occluder BVH on the device (built on the host, host/bvh.cpp).
struct DevBvh {
    DMem<alvrl::BvhNode> nodes;
    DMem<float> tris;
    DMem<uint32_t> ids;
    alvrl::bvh::View view{nullptr, nullptr, nullptr, 0u};
    hipError_t upload(const std::vector<float>& occ)
    {
        const uint32_t nt = (uint32_t)(occ.size() / 9);
        if (nt == 0) return hipSuccess;
        alvrl::BvhHost b;
        try {
            b = alvrl::build_bvh(occ.data(), nt);
        } catch (const std::exception&) {
            return hipErrorInvalidValue;   // deeper than the traversal stacks hold
        }
        hipError_t e = nodes.alloc(b.nodes.size());
        if (e == hipSuccess) e = tris.alloc(b.tris.size());
        if (e == hipSuccess) e = ids.alloc(b.ids.size());
        if (e == hipSuccess) e = hipMemcpy(nodes.p, b.nodes.data(), b.nodes.size() * sizeof(alvrl::BvhNode), hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemcpy(tris.p, b.tris.data(), b.tris.size() * 4, hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemcpy(ids.p, b.ids.data(), b.ids.size() * 4, hipMemcpyHostToDevice);
        if (e == hipSuccess) view = alvrl::bvh::View{nodes.p, tris.p, ids.p, nt};
        return e;
    }
};

// The last BVH built on each device, keyed by the occluder triangles: the
// integrator's calls for one scene (records every render cache refresh and R
// build, the tracer every pass) reuse it instead of rebuilding it each call.
// The cache is never destroyed (its device memory lives until the process
// exits; freeing it from a static destructor could run after the HIP runtime
// is gone); a caller keeps its BVH alive by holding the shared pointer.
std::shared_ptr<DevBvh> cached_bvh(const std::vector<float>& occ, hipError_t* err)
{
    static std::mutex mu;
    static auto* cache = new std::map<int, std::pair<std::vector<float>, std::shared_ptr<DevBvh>>>();
    int dev = 0;
    *err = hipGetDevice(&dev);
    if (*err != hipSuccess) return nullptr;
    std::lock_guard<std::mutex> g(mu);
    auto it = cache->find(dev);
    if (it != cache->end() && it->second.first == occ) return it->second.second;
    auto b = std::make_shared<DevBvh>();
    *err = b->upload(occ);
    if (*err != hipSuccess) return nullptr;
    (*cache)[dev] = {occ, b};
    return b;
}

// Sensor::sampleRay + Scene::rayIntersect (primary_record): the GPU eye-ray
// first hit of SURVEY 8(f) row 1.  pix == nullptr: pixel i.
// spp records per pixel, sample major: record j * n + i is pixel pix[i],
// sensor sample j (its depth word j << 16); spp == 1: pixel centres.
__global__ void __launch_bounds__(256) k_eye_records(Camera c, TScene sc, int scat, const uint32_t* __restrict__ pix,
                                                     uint32_t n, uint32_t spp, uint32_t seed, uint32_t pass,
                                                     float* __restrict__ out)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n * spp) return;
    const uint32_t j = i / n, ii = i - j * n;
    primary_record(sc, c, scat != 0, pix ? pix[ii] : ii, j, spp, seed, pass, out + kRecWords * (size_t)i);
}

// ------------------------------------------------------ eye-path chains --
// chain_walk (transport.h), one lane per pixel, with a capped stack of
// pending siblings per lane; a pixel whose tree needs a deeper one is
// reported (kChainOverflow) and completed by the host's growable stack.
constexpr uint32_t kChainStackDefault = 8u;  // pending siblings per lane
constexpr uint32_t kChainStackMax = 255u;    // a sibling is parked by a node that wrote a record
constexpr int kChainNodeWords = 13;          // p, direction, path weight, throughput, depth

// The pending siblings of lane 'lane' of 'lanes': word w of entry e at
// stack[(e * kChainNodeWords + w) * lanes + lane], so a wave's pushes coalesce.
struct LaneStack {
    float* stack;
    uint64_t lanes, lane;
    uint32_t cap, sp;
    __device__ bool push(const ChainNode& nd)
    {
        if (sp >= cap) return false;   // the entry point completes this pixel on the host
        const float v[kChainNodeWords] = {nd.o.x, nd.o.y, nd.o.z, nd.d.x, nd.d.y, nd.d.z, nd.w[0], nd.w[1], nd.w[2],
                                          nd.thr[0], nd.thr[1], nd.thr[2], __int_as_float(nd.depth)};
#pragma unroll
        for (int w = 0; w < kChainNodeWords; w++) stack[((uint64_t)sp * kChainNodeWords + w) * lanes + lane] = v[w];
        sp++;
        return true;
    }
    __device__ bool pop(ChainNode* nd)
    {
        if (sp == 0) return false;
        --sp;
        float v[kChainNodeWords];
#pragma unroll
        for (int w = 0; w < kChainNodeWords; w++) v[w] = stack[((uint64_t)sp * kChainNodeWords + w) * lanes + lane];
        nd->o = v3(v[0], v[1], v[2]); nd->d = v3(v[3], v[4], v[5]);
        for (int i = 0; i < 3; i++) { nd->w[i] = v[6 + i]; nd->thr[i] = v[9 + i]; }
        nd->depth = __float_as_int(v[12]);
        return true;
    }
};

// Record 0 is the primary record, which k_eye_records writes.  With
// out != nullptr record k >= 1 goes to out[pos[k - 1]] and its source index
// to src[pos[k - 1]], for k < limit only (the pixel's count from the count
// pass: the write pass never leaves the pixel's offsets).
struct LaneOut {
    float* out;
    uint32_t* src;
    const uint32_t* pos;
    uint32_t limit, src_index;
    __device__ float* slot(uint32_t k)
    {
        if (!out || k < 1 || k >= limit) return nullptr;
        const uint32_t d = pos[k - 1];
        src[d] = src_index;
        return out + kRecWords * (size_t)d;
    }
};

// the eye path of pixel i (lane 'lane' of the launch): its number of records, or kChainOverflow
__device__ uint32_t lane_chain(const Camera& c, const TScene& sc, const ChainArgs& a, const uint32_t* pix, uint32_t i,
                               float* stack, uint32_t cap, uint32_t lanes, uint32_t lane, LaneOut out)
{
    const uint32_t id = pix ? pix[i] : i;
    V3 O, D;
    float mint;
    sensor_ray(c, id, a.sample, a.spp, a.seed, a.pass, &O, &D, &mint);
    LaneStack st{stack, lanes, lane, cap, 0u};
    return chain_walk(sc, a, id, O, D, mint, st, out);
}

// count pass: counts[i] = records of pixel i's eye path (kChainOverflow: its
// index is appended to ovf, *n_ovf counting them; at most n)
// One launch covers pixels i0 .. i0 + lanes - 1 (those below n); the stack
// workspace holds 'lanes' lanes.
__global__ void __launch_bounds__(256) k_chain_count(Camera c, TScene sc, ChainArgs a, const uint32_t* __restrict__ pix,
                                                     uint32_t i0, uint32_t lanes, uint32_t n,
                                                     float* __restrict__ stack, uint32_t cap, uint32_t* __restrict__ counts,
                                                     uint32_t* __restrict__ ovf, uint32_t* __restrict__ n_ovf)
{
    const uint32_t lane = blockIdx.x * blockDim.x + threadIdx.x;
    if (lane >= lanes || lane >= n - i0) return;
    const uint32_t i = i0 + lane;
    const uint32_t k = lane_chain(c, sc, a, pix, i, stack, cap, lanes, lane, LaneOut{nullptr, nullptr, nullptr, 0u, i});
    counts[i] = k;
    if (k == kChainOverflow) {
        const uint32_t slot = atomicAdd(n_ovf, 1u);
        if (slot < n) ovf[slot] = i;
    }
}

// write pass: pixel i's records 1..counts[i]-1 at the positions pos[base[i]..]
// the entry point derived from the counts; an overflowed pixel is the host's
__global__ void __launch_bounds__(256) k_chain_write(Camera c, TScene sc, ChainArgs a, const uint32_t* __restrict__ pix,
                                                     uint32_t i0, uint32_t lanes, uint32_t n,
                                                     float* __restrict__ stack, uint32_t cap,
                                                     const uint32_t* __restrict__ counts,
                                                     const uint64_t* __restrict__ base,
                                                     const uint32_t* __restrict__ pos, float* __restrict__ out,
                                                     uint32_t* __restrict__ src)
{
    const uint32_t lane = blockIdx.x * blockDim.x + threadIdx.x;
    if (lane >= lanes || lane >= n - i0) return;
    const uint32_t i = i0 + lane;
    const uint32_t cnt = counts[i];
    if (cnt == kChainOverflow || cnt < 2u) return;
    (void)lane_chain(c, sc, a, pix, i, stack, cap, lanes, lane, LaneOut{out, src, pos + base[i], cnt, i});
}

// the host-completed pixels' records into their places: record j to out[pos[j]]
__global__ void __launch_bounds__(256) k_chain_splice(const float* __restrict__ recs, const uint32_t* __restrict__ pos,
                                                      const uint32_t* __restrict__ srcs, uint32_t m,
                                                      float* __restrict__ out, uint32_t* __restrict__ src)
{
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= m) return;
    const uint32_t d = pos[j];
#pragma unroll
    for (int q = 0; q < 20; q++) out[20 * (size_t)d + q] = recs[20 * (size_t)j + q];
    src[d] = srcs[j];
}

// ----------------------------------------------------- volpath reference --
// VolumetricPathTracer::Li_original with onlyVRLpaths (src/integrators/path/
// volpath.cpp:120-457): the path-traced ground truth of the light transport
// VRLs represent, for the statistical parity of the VRL
// method.  One lane per pixel, its samples in order; draws from the counter
// stream (seed, pass, dom 6, pixel, sample) in the reference's order:
// sampleDistance (1-2), medium NEE (2, when requested), phase sample (2),
// surface NEE (2, when requested), BSDF sample (2), Russian roulette (1).
// Isotropic phase, point light (EDiscrete: every MIS weight is 1), diffuse
// walls and occluders, strictNormals off, no emitter is hit by a ray.
struct VParams {
    int max_depth, rr_depth, only_vrl, vol_to_vol, vol_to_surf;
    float intensity[3];
};

// evalTransmittance(p1, p1OnSurface, light, false) (scene.cpp:619-679):
// medium transmittance over the whole segment, 0 behind an occluder
__device__ void attenuation(const TScene& sc, V3 p1, bool p1_surface, V3 p2, float tr[3])
{
    const V3 d0 = p2 - p1;
    const float remaining = length(d0);
    const float negLength = 0.0f - remaining;
    const float* sigma_t = sc.medium.sigma_t;
    for (int i = 0; i < 3; i++) tr[i] = sigma_t[i] != 0 ? fastexp(sigma_t[i] * negLength) : 1.0f;
    if (sc.bv.ntri && remaining > 0) {
        if (bvh::occluded(sc.bv, p1, d0 * (1.0f / remaining), p1_surface ? 1e-4f : 0.0f, remaining))
            tr[0] = tr[1] = tr[2] = 0.0f;
    }
}

// Scene::sampleAttenuatedEmitterDirect + PointEmitter::sampleDirect
// (scene.cpp:854-898, point.cpp:131-147): value and unit direction to the light
__device__ void light_direct(const TScene& sc, const VParams& vp, V3 ref, bool on_surface, float val[3], V3* dir)
{
    const V3 L = v3(sc.light_pos[0], sc.light_pos[1], sc.light_pos[2]);
    V3 d = L - ref;
    const float dist = length(d);
    const float invDist = 1.0f / dist;
    d = d * invDist;
    *dir = d;
    float tr[3];
    attenuation(sc, ref, on_surface, L, tr);
    for (int i = 0; i < 3; i++) {
        val[i] = vp.intensity[i] * (invDist * invDist);
        val[i] *= tr[i] * 1.0f;   // / emPdf (one emitter)
    }
}

__device__ void volpath_li(const TScene& sc, const VParams& vp, Stream& smp, V3 o, V3 dir, float mint, float Li[3])
{
    const MediumParams& m = sc.medium;
    Li[0] = Li[1] = Li[2] = 0.0f;
    bool first_ok = false, second_ok = false, prev_diffuse = false, prev_volume = false;
    V3 n, hp;
    int hit_tri;
    float its_t = first_hit(sc, o, dir, mint, &n, &hp, &hit_tri);
    float thr[3] = {1.0f, 1.0f, 1.0f};
    const float eta = 1.0f;
    int depth = 1;
    bool indirect = true;   // rRec.type keeps EIndirect*Radiance (ERadiance / ERadianceNoEmission)
    while (depth <= vp.max_depth || vp.max_depth < 0) {
        if (vp.only_vrl && depth > 2 && !(first_ok && second_ok)) break;   // :144-145
        // HomogeneousMedium::sampleDistance over Ray(ray, 0, its.t)
        V3 mp;
        float pf, ps, mtr[3];
        if (m.sample_segment(smp, o, dir, its_t, &mp, &ps, &pf, mtr)) {   // :150-267
            if (depth == 1 && vp.vol_to_vol) first_ok = true;
            if (depth == 2) second_ok = true;
            if (depth >= vp.max_depth && vp.max_depth != -1) break;
            const float rps = 1.0f / ps;
            for (int i = 0; i < 3; i++) thr[i] *= (m.sigma_s[i] * mtr[i]) * rps;
            // luminaire sampling; the reference's "(!rRec.depth==2 || ...)" is
            // "((!depth) == 2 || ...)", i.e. the bracket alone (:183-190)
            const bool nee = !vp.only_vrl ||
                             (depth != 1 && (prev_volume || prev_diffuse) && (!prev_diffuse || vp.vol_to_surf) &&
                              (!prev_volume || vp.vol_to_vol));
            if (nee) {
                (void)smp.next(); (void)smp.next();   // rRec.nextSample2D() (unused by a point light)
                float val[3];
                V3 ld;
                light_direct(sc, vp, mp, false, val, &ld);
                if (!is_zero(val)) {
                    const float phaseVal = 0.079577471545947667884f;   // IsotropicPhaseFunction::eval, 1/(4 pi)
                    for (int i = 0; i < 3; i++) Li[i] += ((thr[i] * val[i]) * phaseVal) * 1.0f;
                }
            }
            // phase sampling (isotropic: weight 1)
            const float px_ = smp.next(), py_ = smp.next();
            const V3 wo = uniform_sphere(px_, py_);
            o = mp; dir = wo;
            its_t = first_hit(sc, o, dir, 0.0f, &n, &hp, &hit_tri);
            if (!indirect) break;
            prev_volume = true;
            prev_diffuse = false;
        } else {   // :268-435
            const float rpf = 1.0f / pf;
            for (int i = 0; i < 3; i++) thr[i] *= mtr[i] * rpf;
            if (!isfinite(its_t)) break;
            if (depth >= vp.max_depth && vp.max_depth != -1) break;
            const float* alb = sc.albedo_of(hit_tri);
            const V3 p = hp;
            const float cos_wi = dot(-dir, n);
            if (!vp.only_vrl || (first_ok && second_ok)) {   // :319-350 (ESmooth diffuse)
                (void)smp.next(); (void)smp.next();
                float val[3];
                V3 ld;
                light_direct(sc, vp, p, true, val, &ld);
                if (!is_zero(val)) {
                    const float cos_wo = dot(ld, n);
                    if (!(cos_wi <= 0 || cos_wo <= 0)) {
                        const float k = 0.31830988618379067154f * cos_wo;   // INV_PI * cosTheta(wo)
                        for (int i = 0; i < 3; i++) Li[i] += ((thr[i] * val[i]) * (alb[i] * k)) * 1.0f;
                    }
                }
            }
            // BSDF sampling (diffuse.cpp:140-150)
            const float bx = smp.next(), by = smp.next();
            if (cos_wi <= 0) break;   // bsdfWeight.isZero()
            const V3 wo = frame_of(n).to_world(cosine_hemisphere(bx, by));
            if (depth == 1 && vp.vol_to_surf) first_ok = true;   // :377-382 (inside the medium, smooth)
            prev_volume = false;
            prev_diffuse = true;
            for (int i = 0; i < 3; i++) thr[i] *= alb[i];
            o = p; dir = wo;
            its_t = first_hit(sc, o, dir, 1e-4f, &n, &hp, &hit_tri);
            if (!indirect) break;
        }
        if (depth++ >= vp.rr_depth) {   // :437-446
            float q = max3(thr) * eta * eta;
            if (q > 0.95f) q = 0.95f;
            if (smp.next() >= q) break;
            const float rq = 1.0f / q;
            for (int i = 0; i < 3; i++) thr[i] *= rq;
        }
    }
    if (vp.only_vrl && !(first_ok && second_ok)) Li[0] = Li[1] = Li[2] = 0.0f;   // :453-455
}

__global__ void __launch_bounds__(256) k_volpath(Camera c, TScene sc, VParams vp, uint32_t seed, uint32_t pass,
                                                 uint32_t spp, const uint32_t* __restrict__ pix, uint32_t n,
                                                 float* __restrict__ out)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t id = pix ? pix[i] : i;
    V3 O, D;
    float mint;
    sensor_ray(c, id, 0u, 1u, seed, pass, &O, &D, &mint);   // the pixel centre
    float acc[3] = {0.0f, 0.0f, 0.0f};
    for (uint32_t s = 0; s < spp; s++) {
        Stream smp(seed, pass, kDomVolpath, id, s);
        float li[3];
        volpath_li(sc, vp, smp, O, D, mint, li);
        for (int k = 0; k < 3; k++) acc[k] += li[k];
    }
    const float r = 1.0f / (float)spp;
    for (int k = 0; k < 3; k++) out[3 * (size_t)i + k] = acc[k] * r;
}

// the host's view of the scene, its tables not yet on the device: the caller
// uploads them (cached_bvh, upload_albedos, upload_materials, the emitter)
TScene make_tscene(const alvrl::host::SmokeBox& box)
{
    TScene sc;
    static_cast<SceneView&>(sc) = box.view();
    sc.occ_alb = nullptr;
    sc.occ_mat = nullptr;
    sc.emit = nullptr;
    sc.emit_cdf = nullptr;
    sc.bv = alvrl::bvh::View{nullptr, nullptr, nullptr, 0u};
    return sc;
}

}  // namespace

extern "C" {

ALVRL_API void alvrl_volpath_default(alvrl_volpath_params* p)
{
    if (!p) return;
    p->max_depth = -1;       // MonteCarloIntegrator maxDepth
    p->rr_depth = 5;         // rrDepth
    p->only_vrl_paths = 1;   // volpath.cpp:79-81
    p->vrl_vol_to_vol = 1;
    p->vrl_vol_to_surf = 1;
}

// the occluders' own reflectances on the device (SmokeBox::occ_alb), for TScene::occ_alb
static bool upload_albedos(const alvrl::host::SmokeBox& box, DMem<float>& d, TScene& sc)
{
    if (box.occ_alb.empty()) return true;
    if (d.alloc(box.occ_alb.size()) != hipSuccess) return false;
    if (hipMemcpy(d.p, box.occ_alb.data(), box.occ_alb.size() * 4, hipMemcpyHostToDevice) != hipSuccess) return false;
    sc.occ_alb = d.p;
    return true;
}

// the occluders' BSDFs on the device (SmokeBox::occ_mat), for TScene::occ_mat
static bool upload_materials(const alvrl::host::SmokeBox& box, DMem<uint32_t>& d, TScene& sc)
{
    if (!box.has_delta()) return true;   // all diffuse: no table
    if (d.alloc(box.occ_mat.size()) != hipSuccess) return false;
    if (hipMemcpy(d.p, box.occ_mat.data(), box.occ_mat.size() * 4, hipMemcpyHostToDevice) != hipSuccess) return false;
    sc.occ_mat = d.p;
    return true;
}

ALVRL_API int alvrl_volpath_render(const alvrl_scene_desc* s, const alvrl_volpath_params* p, uint32_t seed,
                                   uint32_t pass, uint32_t spp, const uint32_t* d_pixel_ids, uint32_t n,
                                   float* d_out_rgb, void* stream)
{
    if (!s || !p || (!d_out_rgb && n)) return terr(ALVRL_ERR_INVALID, "alvrl_volpath_render: null argument");
    if (spp == 0) return terr(ALVRL_ERR_INVALID, "alvrl_volpath_render: spp must be > 0");
    if (s->medium.phase_type != 0)
        return terr(ALVRL_ERR_INVALID, "alvrl_volpath_render: only the isotropic phase function is supported");
    if (const char* m = alvrl::host::scene_problem(*s)) return terr(ALVRL_ERR_INVALID, m);
    const alvrl::host::SmokeBox box = alvrl::host::to_box(*s);
    if (box.has_delta())
        return terr(ALVRL_ERR_INVALID, "alvrl_volpath_render: mirror / null occluders are not supported by the volpath reference");
    if (box.area_light())
        return terr(ALVRL_ERR_INVALID, "alvrl_volpath_render: the volpath reference samples the point light only");
    const uint64_t npix = (uint64_t)box.width * (uint64_t)box.height;
    if (!d_pixel_ids && n > npix) return terr(ALVRL_ERR_INVALID, "alvrl_volpath_render: n > W*H without pixel ids");
    if (n == 0) return ALVRL_OK;
    TScene sc = make_tscene(box);
    hipError_t be = hipSuccess;
    const std::shared_ptr<DevBvh> bv = cached_bvh(box.occ, &be);
    if (!bv) return terr(ALVRL_ERR_HIP, "alvrl_volpath_render: BVH upload");
    sc.bv = bv->view;
    DMem<float> d_alb;
    if (!upload_albedos(box, d_alb, sc)) return terr(ALVRL_ERR_HIP, "alvrl_volpath_render: albedo upload");
    const Camera c = box.camera();
    VParams vp;
    vp.max_depth = p->max_depth; vp.rr_depth = p->rr_depth; vp.only_vrl = p->only_vrl_paths ? 1 : 0;
    vp.vol_to_vol = p->vrl_vol_to_vol ? 1 : 0; vp.vol_to_surf = p->vrl_vol_to_surf ? 1 : 0;
    for (int i = 0; i < 3; i++) vp.intensity[i] = box.light_intensity[i];
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_volpath, dim3((n + 255) / 256), dim3(256), 0, st, c, sc, vp, seed, pass, spp, d_pixel_ids, n,
                       d_out_rgb);
    if (hipGetLastError() != hipSuccess) return terr(ALVRL_ERR_HIP, "alvrl_volpath_render: launch");
    if (hipStreamSynchronize(st) != hipSuccess) return terr(ALVRL_ERR_HIP, "alvrl_volpath_render: sync");
    return ALVRL_OK;
}

// Gather records of pixel centres on the current HIP device (the host
// alvrl_scene_records, bit for bit).  d_pixel_ids (device, row-major y*W+x)
// may be NULL: pixels 0..n-1.  d_out: n device records.  Stream-ordered on
// 'stream' (the occluder BVH is built and uploaded synchronously first).
ALVRL_API int alvrl_scene_records_gpu(const alvrl_scene_desc* s, int medium_scatters, const uint32_t* d_pixel_ids,
                                      uint32_t n, alvrl_gather_rec* d_out, void* stream)
{
    return alvrl_scene_records_spp_gpu(s, medium_scatters, 0u, 0u, 1u, d_pixel_ids, n, d_out, stream);
}

// The sensor samples of alvrl_scene_records_spp (the host's, bit for bit):
// n * spp device records, sample major.
ALVRL_API int alvrl_scene_records_spp_gpu(const alvrl_scene_desc* s, int medium_scatters, uint32_t seed,
                                          uint32_t pass, uint32_t spp, const uint32_t* d_pixel_ids, uint32_t n,
                                          alvrl_gather_rec* d_out, void* stream)
{
    if (!s || (!d_out && n)) return terr(ALVRL_ERR_INVALID, "alvrl_scene_records_gpu: null argument");
    if (spp == 0 || spp > 0xFFFFu || (uint64_t)spp * n > 0xFFFFFFFFull)
        return terr(ALVRL_ERR_INVALID, "alvrl_scene_records_spp_gpu: spp out of range");
    if (const char* m = alvrl::host::scene_problem(*s)) return terr(ALVRL_ERR_INVALID, m);
    const alvrl::host::SmokeBox box = alvrl::host::to_box(*s);
    const uint64_t npix = (uint64_t)box.width * (uint64_t)box.height;
    if (!d_pixel_ids && n > npix) return terr(ALVRL_ERR_INVALID, "alvrl_scene_records_gpu: n > W*H without pixel ids");
    if (n == 0) return ALVRL_OK;
    TScene sc = make_tscene(box);
    hipError_t be = hipSuccess;
    const std::shared_ptr<DevBvh> bv = cached_bvh(box.occ, &be);
    if (!bv) return terr(ALVRL_ERR_HIP, "alvrl_scene_records_gpu: BVH upload");
    sc.bv = bv->view;
    DMem<float> d_alb;
    if (!upload_albedos(box, d_alb, sc)) return terr(ALVRL_ERR_HIP, "alvrl_scene_records_gpu: albedo upload");
    DMem<uint32_t> d_mat;
    if (!upload_materials(box, d_mat, sc)) return terr(ALVRL_ERR_HIP, "alvrl_scene_records_gpu: material upload");
    const Camera c = box.camera();
    const int scat = medium_scatters && sc.medium.scatters() ? 1 : 0;
    hipStream_t st = (hipStream_t)stream;
    const uint32_t total = n * spp;
    hipLaunchKernelGGL(k_eye_records, dim3((total + 255) / 256), dim3(256), 0, st, c, sc, scat, d_pixel_ids, n, spp, seed,
                       pass, reinterpret_cast<float*>(d_out));
    if (hipGetLastError() != hipSuccess) return terr(ALVRL_ERR_HIP, "alvrl_scene_records_gpu: launch");
    // stream-ordered callers may replace the cached BVH after return: wait for the kernel
    if (hipStreamSynchronize(st) != hipSuccess) return terr(ALVRL_ERR_HIP, "alvrl_scene_records_gpu: sync");
    return ALVRL_OK;
}

// The device form of alvrl_scene_chain_spp for n pixels (include/alvrl_host.h).
// Count pass, then the offsets on the host (per level, in pixel order), then
// the write pass; pixels the count pass reports as overflowed are completed
// by SmokeBox::make_chain and spliced in.
ALVRL_API int alvrl_scene_chains_gpu(const alvrl_scene_desc* s, int medium_scatters, uint32_t seed, uint32_t pass,
                                     int spec_rr_depth, float init_throughput, uint32_t sample, uint32_t spp,
                                     const uint32_t* d_pixel_ids, uint32_t n, uint32_t stack_cap,
                                     uint32_t* d_counts, uint32_t* level_off, uint32_t* n_levels,
                                     alvrl_gather_rec* d_recs, uint32_t* d_src, uint64_t cap, uint64_t* total,
                                     uint32_t* n_overflow, void* stream)
{
    if (!s || !level_off || !n_levels || !total || (d_recs && !d_src))
        return terr(ALVRL_ERR_INVALID, "alvrl_scene_chains_gpu: null argument");
    if (spp == 0 || sample >= spp || spp > 0xFFFFu)
        return terr(ALVRL_ERR_INVALID, "alvrl_scene_chains_gpu: sample out of range");
    if (const char* m = alvrl::host::scene_problem(*s)) return terr(ALVRL_ERR_INVALID, m);
    const alvrl::host::SmokeBox box = alvrl::host::to_box(*s);
    const uint64_t npix = (uint64_t)box.width * (uint64_t)box.height;
    if (!d_pixel_ids && n > npix) return terr(ALVRL_ERR_INVALID, "alvrl_scene_chains_gpu: n > W*H without pixel ids");
    for (uint32_t d = 0; d <= ALVRL_CHAIN_MAX_LEVELS; d++) level_off[d] = 0;
    *n_levels = 0;
    *total = 0;
    if (n_overflow) *n_overflow = 0;
    if (n == 0) return ALVRL_OK;
    TScene sc = make_tscene(box);
    hipError_t be = hipSuccess;
    const std::shared_ptr<DevBvh> bv = cached_bvh(box.occ, &be);
    if (!bv) return terr(ALVRL_ERR_HIP, "alvrl_scene_chains_gpu: BVH upload");
    sc.bv = bv->view;
    DMem<float> d_alb;
    if (!upload_albedos(box, d_alb, sc)) return terr(ALVRL_ERR_HIP, "alvrl_scene_chains_gpu: albedo upload");
    DMem<uint32_t> d_mat;
    if (!upload_materials(box, d_mat, sc)) return terr(ALVRL_ERR_HIP, "alvrl_scene_chains_gpu: material upload");
    const bool scat = medium_scatters && sc.medium.scatters();
    const Camera c = box.camera();
    ChainArgs a;
    a.seed = seed; a.pass = pass; a.sample = sample; a.spp = spp;
    a.flags = 1u | (scat ? 4u : 0u);
    const uint32_t stack_entries = stack_cap ? std::min(stack_cap, kChainStackMax) : kChainStackDefault;   // per lane
    a.spec_rr_depth = spec_rr_depth;
    a.init_thr = init_throughput;
    hipStream_t st = (hipStream_t)stream;
    // the stack workspace serves one launch of at most 2^18 lanes at a time
    const uint32_t lanes = std::min<uint32_t>(n, 1u << 18);
    DMem<float> d_stack;
    DMem<uint32_t> d_cnt, d_ovf, d_novf;
    if (d_stack.alloc((size_t)lanes * stack_entries * kChainNodeWords) != hipSuccess || d_cnt.alloc(n) != hipSuccess ||
        d_ovf.alloc(n) != hipSuccess || d_novf.alloc(1) != hipSuccess)
        return terr(ALVRL_ERR_NOMEM, "alvrl_scene_chains_gpu: device memory");
    if (hipMemsetAsync(d_novf.p, 0, 4, st) != hipSuccess) return terr(ALVRL_ERR_HIP, "alvrl_scene_chains_gpu: clear");
    for (uint32_t i0 = 0; i0 < n; i0 += lanes) {
        hipLaunchKernelGGL(k_chain_count, dim3((lanes + 255) / 256), dim3(256), 0, st, c, sc, a, d_pixel_ids, i0, lanes, n,
                           d_stack.p, stack_entries, d_cnt.p, d_ovf.p, d_novf.p);
        if (hipGetLastError() != hipSuccess) return terr(ALVRL_ERR_HIP, "alvrl_scene_chains_gpu: launch");
    }
    std::vector<uint32_t> counts(n);
    uint32_t novf = 0;
    if (hipMemcpyAsync(counts.data(), d_cnt.p, (size_t)n * 4, hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipMemcpyAsync(&novf, d_novf.p, 4, hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipStreamSynchronize(st) != hipSuccess)
        return terr(ALVRL_ERR_HIP, "alvrl_scene_chains_gpu: count pass");
    novf = std::min(novf, n);
    // the overflowed pixels' whole eye paths from the host (record 0 included)
    std::vector<uint32_t> ovf(novf);
    std::vector<std::vector<float>> ovf_recs(novf);
    if (novf) {
        if (hipMemcpy(ovf.data(), d_ovf.p, (size_t)novf * 4, hipMemcpyDeviceToHost) != hipSuccess)
            return terr(ALVRL_ERR_HIP, "alvrl_scene_chains_gpu: copy");
        std::sort(ovf.begin(), ovf.end());
        std::vector<uint32_t> ids;
        if (d_pixel_ids) {
            ids.resize(n);
            if (hipMemcpy(ids.data(), d_pixel_ids, (size_t)n * 4, hipMemcpyDeviceToHost) != hipSuccess)
                return terr(ALVRL_ERR_HIP, "alvrl_scene_chains_gpu: copy");
        }
        const uint32_t W = (uint32_t)box.width;
        for (uint32_t j = 0; j < novf; j++) {
            const uint32_t id = d_pixel_ids ? ids[ovf[j]] : ovf[j];
            box.make_chain((int)(id % W), (int)(id / W), scat, seed, pass, spec_rr_depth, init_throughput, &ovf_recs[j],
                           sample, spp);
            counts[ovf[j]] = (uint32_t)(ovf_recs[j].size() / kRecWords);
        }
    }
    if (n_overflow) *n_overflow = novf;
    // level d holds record d + 1 of every pixel that has one, in pixel order
    uint64_t hist[kChainMaxRecs + 1] = {0};
    for (uint32_t i = 0; i < n; i++) hist[std::min(counts[i], kChainMaxRecs)]++;
    uint64_t tot = 0, above = 0;
    uint64_t lv[ALVRL_CHAIN_MAX_LEVELS + 1];
    for (uint32_t d = ALVRL_CHAIN_MAX_LEVELS; d-- > 0;) {   // pixels with more than d + 1 records
        above += hist[d + 2];
        lv[d] = above;
    }
    uint32_t nl = 0;
    for (uint32_t d = 0; d < ALVRL_CHAIN_MAX_LEVELS; d++) {
        if (lv[d]) nl = d + 1;
        tot += lv[d];
    }
    *total = tot;
    if (tot > 0xFFFFFFFFull) return terr(ALVRL_ERR_INVALID, "alvrl_scene_chains_gpu: more than 2^32 records");
    uint64_t run = 0;
    for (uint32_t d = 0; d < ALVRL_CHAIN_MAX_LEVELS; d++) { level_off[d] = (uint32_t)run; run += lv[d]; }
    level_off[ALVRL_CHAIN_MAX_LEVELS] = (uint32_t)run;
    *n_levels = nl;
    if (d_counts && hipMemcpy(d_counts, counts.data(), (size_t)n * 4, hipMemcpyHostToDevice) != hipSuccess)
        return terr(ALVRL_ERR_HIP, "alvrl_scene_chains_gpu: copy");
    if (!d_recs) return ALVRL_OK;   // size query
    if (tot > cap) return terr(ALVRL_ERR_INVALID, "alvrl_scene_chains_gpu: capacity too small");
    if (tot == 0) return ALVRL_OK;
    // pos[base[i] + k - 1]: where record k of pixel i goes
    std::vector<uint64_t> base(n);
    std::vector<uint32_t> pos((size_t)tot), fill(level_off, level_off + ALVRL_CHAIN_MAX_LEVELS);
    uint64_t b = 0;
    for (uint32_t i = 0; i < n; i++) {
        base[i] = b;
        for (uint32_t k = 1; k < counts[i]; k++) pos[(size_t)b++] = fill[k - 1]++;
    }
    DMem<uint64_t> d_base;
    DMem<uint32_t> d_pos;
    if (d_base.alloc(n) != hipSuccess || d_pos.alloc((size_t)tot) != hipSuccess)
        return terr(ALVRL_ERR_NOMEM, "alvrl_scene_chains_gpu: device memory");
    if (hipMemcpyAsync(d_base.p, base.data(), (size_t)n * 8, hipMemcpyHostToDevice, st) != hipSuccess ||
        hipMemcpyAsync(d_pos.p, pos.data(), (size_t)tot * 4, hipMemcpyHostToDevice, st) != hipSuccess)
        return terr(ALVRL_ERR_HIP, "alvrl_scene_chains_gpu: copy");
    // d_cnt keeps kChainOverflow for the host's pixels: the write pass skips them
    for (uint32_t i0 = 0; i0 < n; i0 += lanes) {
        hipLaunchKernelGGL(k_chain_write, dim3((lanes + 255) / 256), dim3(256), 0, st, c, sc, a, d_pixel_ids, i0, lanes, n,
                           d_stack.p, stack_entries, d_cnt.p, d_base.p, d_pos.p, reinterpret_cast<float*>(d_recs), d_src);
        if (hipGetLastError() != hipSuccess) return terr(ALVRL_ERR_HIP, "alvrl_scene_chains_gpu: launch");
    }
    DMem<float> d_hrec;
    DMem<uint32_t> d_hpos, d_hsrc;
    std::vector<float> hrec;
    std::vector<uint32_t> hpos, hsrc;
    for (uint32_t j = 0; j < novf; j++) {
        const uint32_t i = ovf[j];
        for (uint32_t k = 1; k < counts[i]; k++) {
            hrec.insert(hrec.end(), ovf_recs[j].begin() + (size_t)k * kRecWords,
                        ovf_recs[j].begin() + (size_t)(k + 1) * kRecWords);
            hpos.push_back(pos[(size_t)base[i] + k - 1]);
            hsrc.push_back(i);
        }
    }
    if (!hpos.empty()) {
        const uint32_t m = (uint32_t)hpos.size();
        if (d_hrec.alloc(hrec.size()) != hipSuccess || d_hpos.alloc(m) != hipSuccess || d_hsrc.alloc(m) != hipSuccess)
            return terr(ALVRL_ERR_NOMEM, "alvrl_scene_chains_gpu: device memory");
        if (hipMemcpyAsync(d_hrec.p, hrec.data(), hrec.size() * 4, hipMemcpyHostToDevice, st) != hipSuccess ||
            hipMemcpyAsync(d_hpos.p, hpos.data(), (size_t)m * 4, hipMemcpyHostToDevice, st) != hipSuccess ||
            hipMemcpyAsync(d_hsrc.p, hsrc.data(), (size_t)m * 4, hipMemcpyHostToDevice, st) != hipSuccess)
            return terr(ALVRL_ERR_HIP, "alvrl_scene_chains_gpu: copy");
        hipLaunchKernelGGL(k_chain_splice, dim3((m + 255) / 256), dim3(256), 0, st, d_hrec.p, d_hpos.p, d_hsrc.p, m,
                           reinterpret_cast<float*>(d_recs), d_src);
        if (hipGetLastError() != hipSuccess) return terr(ALVRL_ERR_HIP, "alvrl_scene_chains_gpu: launch");
    }
    // the workspace and the cached BVH may go after return: wait for the kernels
    if (hipStreamSynchronize(st) != hipSuccess) return terr(ALVRL_ERR_HIP, "alvrl_scene_chains_gpu: sync");
    return ALVRL_OK;
}

// The GPU form of alvrl_trace_vrls (same arguments and results); runs on the
// current HIP device.
ALVRL_API int alvrl_trace_vrls_gpu(const alvrl_scene_desc* s, uint32_t seed, uint32_t pass, uint32_t target,
                                   int short_vrls, int max_depth, int rr_depth, float* soa, uint32_t cap,
                                   uint32_t* n, uint64_t* particles)
{
    if (!s || !n || !particles) return terr(ALVRL_ERR_INVALID, "alvrl_trace_vrls_gpu: null argument");
    // the scene as the host tracer resolves it (to_box + MediumParams::resolve)
    if (const char* m = alvrl::host::scene_problem(*s)) return terr(ALVRL_ERR_INVALID, m);
    const alvrl::host::SmokeBox box = alvrl::host::to_box(*s);
    TScene sc = make_tscene(box);
    hipError_t be = hipSuccess;
    const std::shared_ptr<DevBvh> bvh = cached_bvh(box.occ, &be);
    if (!bvh) return terr(ALVRL_ERR_HIP, "alvrl_trace_vrls_gpu: BVH upload");
    sc.bv = bvh->view;
    DMem<float> d_alb;
    if (!upload_albedos(box, d_alb, sc)) return terr(ALVRL_ERR_HIP, "alvrl_trace_vrls_gpu: albedo upload");
    DMem<uint32_t> d_mat;
    if (!upload_materials(box, d_mat, sc)) return terr(ALVRL_ERR_HIP, "alvrl_trace_vrls_gpu: material upload");
    const TArgs a{seed, pass, short_vrls, max_depth, rr_depth};
    *n = 0;
    if (target == 0) { *particles = 0; return ALVRL_OK; }
    if (!sc.medium.scatters()) { *particles = 1000001; return ALVRL_OK; }   // the host loop's bound
    const float* pw = sc.nemit ? sc.emit_radiance : sc.power;
    if (pw[0] == 0 && pw[1] == 0 && pw[2] == 0)
        return terr(ALVRL_ERR_INVALID, "alvrl_trace_vrls_gpu: the light emits nothing (the VRL target is unreachable)");
    // the area emitter's triangles and sampling table on the device
    DMem<float> d_emit, d_cdf;
    if (sc.nemit) {
        if (d_emit.alloc(box.emit.size()) != hipSuccess || d_cdf.alloc(box.emit_cdf.size()) != hipSuccess)
            return terr(ALVRL_ERR_NOMEM, "alvrl_trace_vrls_gpu: device memory");
        if (hipMemcpy(d_emit.p, box.emit.data(), box.emit.size() * 4, hipMemcpyHostToDevice) != hipSuccess ||
            hipMemcpy(d_cdf.p, box.emit_cdf.data(), box.emit_cdf.size() * 4, hipMemcpyHostToDevice) != hipSuccess)
            return terr(ALVRL_ERR_HIP, "alvrl_trace_vrls_gpu: copy");
        sc.emit = d_emit.p;
        sc.emit_cdf = d_cdf.p;
    }
    // count pass, batch by batch, until the running total reaches the target
    const uint32_t P = std::min<uint32_t>(1u << 20, std::max<uint32_t>(4096u, target));
    DMem<uint32_t> d_cnt;
    if (d_cnt.alloc(P) != hipSuccess) return terr(ALVRL_ERR_NOMEM, "alvrl_trace_vrls_gpu: device memory");
    std::vector<uint32_t> counts;
    uint64_t total = 0, used = 0;
    for (uint64_t p0 = 0; used == 0; p0 += P) {
        if (p0 > (1ull << 32)) return terr(ALVRL_ERR_INVALID, "alvrl_trace_vrls_gpu: target not reached");
        hipLaunchKernelGGL(k_trace_count, dim3((P + 255) / 256), dim3(256), 0, 0, sc, a, p0, P, d_cnt.p);
        if (hipGetLastError() != hipSuccess) return terr(ALVRL_ERR_HIP, "alvrl_trace_vrls_gpu: launch");
        const size_t base = counts.size();
        counts.resize(base + P);
        if (hipMemcpy(counts.data() + base, d_cnt.p, P * 4, hipMemcpyDeviceToHost) != hipSuccess)
            return terr(ALVRL_ERR_HIP, "alvrl_trace_vrls_gpu: copy");
        for (uint32_t i = 0; i < P; i++) {
            total += counts[base + i];
            if (total >= target) { used = base + i + 1; break; }
        }
    }
    *particles = used;
    *n = (uint32_t)total;
    if (!soa) return ALVRL_OK;   // size query
    if (total > cap) return terr(ALVRL_ERR_INVALID, "alvrl_trace_vrls_gpu: capacity too small");
    // write pass: every particle's VRLs at its exclusive prefix offset
    std::vector<uint64_t> offs(used);
    uint64_t o = 0;
    for (uint64_t i = 0; i < used; i++) { offs[i] = o; o += counts[i]; }
    DMem<uint64_t> d_off;
    DMem<float> d_soa;
    if (d_off.alloc(used) != hipSuccess || d_soa.alloc(9 * total) != hipSuccess)
        return terr(ALVRL_ERR_NOMEM, "alvrl_trace_vrls_gpu: device memory");
    if (hipMemcpy(d_off.p, offs.data(), used * 8, hipMemcpyHostToDevice) != hipSuccess)
        return terr(ALVRL_ERR_HIP, "alvrl_trace_vrls_gpu: copy");
    for (uint64_t p0 = 0; p0 < used; p0 += P) {
        const uint32_t np = (uint32_t)std::min<uint64_t>(P, used - p0);
        hipLaunchKernelGGL(k_trace_write, dim3((np + 255) / 256), dim3(256), 0, 0, sc, a, p0, np, d_off.p + p0,
                           d_soa.p, total);
        if (hipGetLastError() != hipSuccess) return terr(ALVRL_ERR_HIP, "alvrl_trace_vrls_gpu: launch");
    }
    if (hipMemcpy2D(soa, (size_t)cap * 4, d_soa.p, total * 4, total * 4, 9, hipMemcpyDeviceToHost) != hipSuccess)
        return terr(ALVRL_ERR_HIP, "alvrl_trace_vrls_gpu: copy");
    return ALVRL_OK;
}

}  // extern "C"
