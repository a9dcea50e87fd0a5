// tracer.hip -- vrlTracer::randomWalk (vrlTracer.h:13-230) on the GPU,
// SURVEY.md 8(f) row 2.  One lane per particle: particle p draws from its own
// counter-based stream (seed, pass, p), exactly as the host tracer
// (csrc/host/scene.cpp trace_particle) and the oracle do, so the VRL set is
// the host's bit for bit -- diffuse, mirror, null and dielectric surfaces alike.  Built with -ffp-contract=off and IEEE division /
// square root like the host; sin, cos, exp and log are evaluated in double
// and rounded once, as on the host.
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
#include "detmath.h"

namespace alvrl {
namespace host {
extern thread_local std::string g_host_err;
SmokeBox to_box(const alvrl_scene_desc& s);   // host_capi.cpp
const char* scene_problem(const alvrl_scene_desc& s);
}
}  // namespace alvrl

namespace {

constexpr double kPi = 3.14159265358979323846;
constexpr uint32_t kDomTracer = 3u;

struct TScene {
    float light_pos[3], power[3];
    float box_min[3], box_max[3], albedo[3];
    float sigma_s[3], sigma_t[3], w;
    int strategy;                 // the medium's sampling strategy (MediumParams)
    float density, mx_sigma[3], mx_cdf[4], mx_start[3], mx_lower[3], mx_norm, mx_inv_norm;
    int sigma_s_zero;
    alvrl::bvh::View bv;          // occluders (ntri == 0: none)
    float occ_albedo[3];
    const float* occ_alb;         // per-triangle reflectance (3 floats, by triangle index), or nullptr
    // delta BSDFs (SmokeBox::occ_mat / occ_spec / occ_eta): the per-triangle
    // ALVRL_MAT_* table on the device (nullptr: every triangle diffuse), the
    // mirrors' reflectance, the dielectrics' intIOR / extIOR
    const uint32_t* occ_mat;
    float occ_spec[3], occ_eta;
    // area emitter (SmokeBox::emit; nemit == 0: the point light): triangles,
    // the normalized area CDF (nemit + 1 entries), radiance and surface area
    const float* emit;
    const float* emit_cdf;
    uint32_t nemit;
    float emit_radiance[3], emit_area;
};

struct F3 { float x, y, z; };
__device__ __forceinline__ F3 f3(float x, float y, float z) { return F3{x, y, z}; }
__device__ __forceinline__ F3 add(F3 a, F3 b) { return f3(a.x + b.x, a.y + b.y, a.z + b.z); }
__device__ __forceinline__ F3 sub(F3 a, F3 b) { return f3(a.x - b.x, a.y - b.y, a.z - b.z); }
__device__ __forceinline__ F3 mul(F3 a, float s) { return f3(a.x * s, a.y * s, a.z * s); }
__device__ __forceinline__ float dot(F3 a, F3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__device__ __forceinline__ float len(F3 a) { return sqrtf(a.x * a.x + a.y * a.y + a.z * a.z); }
__device__ __forceinline__ F3 cross(F3 a, F3 b)
{
    return f3(a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x);
}
__device__ __forceinline__ float safe_sqrt(float v) { return sqrtf(v > 0.0f ? v : 0.0f); }
// math::fastexp / fastlog (math.h:185-199): detmath.h, bit for bit the host's and the oracle's
__device__ __forceinline__ float fastexp(float v) { return dm_expf(v); }
__device__ __forceinline__ float fastlog(float v) { return dm_logf(v); }

// HomogeneousMedium::sampleDistance (homogeneous.cpp:275-352) as the host's
// MediumParams / sample_distance: the same float operations, so the same
// values.  'maximum' follows MaxExpDist (maxexp.h:59-94).
__device__ __forceinline__ int interval_of(const float* a, int n, float x)
{
    int k = 0;
    while (k < n && a[k] < x) k++;
    return k > 0 ? k - 1 : 0;
}

__device__ __forceinline__ float maxexp_sample(const TScene& sc, float u, float* pdf)
{
    const int i = min(interval_of(sc.mx_cdf, 4, u), 2);
    const float t = -fastlog(fastexp(-sc.mx_start[i] * sc.mx_sigma[i]) - sc.mx_norm * (u - sc.mx_cdf[i])) / sc.mx_sigma[i];
    *pdf = sc.mx_sigma[i] * fastexp(-sc.mx_sigma[i] * t) * sc.mx_inv_norm;
    return t;
}

__device__ __forceinline__ float maxexp_cdf(const TScene& sc, float t)
{
    const int i = interval_of(sc.mx_start, 3, t);
    const float upper = -fastexp(-sc.mx_sigma[i] * t);
    return sc.mx_cdf[i] + (upper - sc.mx_lower[i]) * sc.mx_inv_norm;
}

__device__ __forceinline__ void medium_pdfs(const TScene& sc, float sampled, float pdf_max, float* ps, float* pf)
{
    const float w = sc.w;
    float s = 0.0f, f = 0.0f;
    if (sc.strategy == 3) {
        f = 1 - maxexp_cdf(sc, sampled);
        s = pdf_max;
    } else if (sc.strategy == 0) {
        for (int i = 0; i < 3; i++) {
            const float tmp = fastexp(-sc.sigma_t[i] * sampled);
            f += tmp;
            s += sc.sigma_t[i] * tmp;
        }
        f /= 3; s /= 3;
    } else {
        f = fastexp(-sc.density * sampled);
        s = sc.density * f;
    }
    *ps = s * w;
    *pf = w * f + (1 - w);
}

// Random123 Philox4x32-10 and Random::nextFloat (random.cpp:630-639), as the host
struct Stream {
    uint32_t seed, pass, a, b, k, blk;
    uint32_t buf[4];
    __device__ float next()
    {
        const uint32_t bl = k >> 2;
        if (bl != blk) {
            uint32_t c0 = a, c1 = b, c2 = bl, c3 = (kDomTracer << 24);
            uint32_t k0 = seed, k1 = pass;
            for (int r = 0; r < 10; r++) {
                if (r > 0) { k0 += 0x9E3779B9u; k1 += 0xBB67AE85u; }
                const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
                const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
                c0 = n0; c1 = (uint32_t)p1; c2 = n2; c3 = (uint32_t)p0;
            }
            buf[0] = c0; buf[1] = c1; buf[2] = c2; buf[3] = c3;
            blk = bl;
        }
        const uint32_t u = (buf[k & 3] >> 9) | 0x3f800000u;
        ++k;
        return __uint_as_float(u) - 1.0f;
    }
};

// sampleDistance's draws (homogeneous.cpp:277-296): the distance (INFINITY:
// no medium interaction) and, for 'maximum', the pdf of the sample
template <class S>
__device__ __forceinline__ float sample_distance(const TScene& sc, S& smp, float* pdf_max)
{
    float rnd = smp.next();
    const float w = sc.w;
    if (!(rnd < w)) return INFINITY;
    rnd /= w;
    if (sc.strategy == 3) return maxexp_sample(sc, 1 - rnd, pdf_max);
    float density = sc.density;
    if (sc.strategy == 0) {   // a random channel each time
        int ch = (int)(smp.next() * 3);
        if (ch > 2) ch = 2;
        density = sc.sigma_t[ch];
    }
    return -fastlog(1 - rnd) / density;
}

__device__ F3 uniform_sphere(float sx, float sy)   // warp.cpp:25-31
{
    const float z = 1.0f - 2.0f * sy;
    const float r = safe_sqrt(1.0f - z * z);
    const float theta = (float)(2.0f * kPi * sx);
    return f3(r * (float)cos((double)theta), r * (float)sin((double)theta), z);
}

__device__ F3 cosine_hemisphere(float sx, float sy)   // warp.cpp:43-52, 81-102
{
    const float r1 = 2.0f * sx - 1.0f, r2 = 2.0f * sy - 1.0f;
    float phi, r;
    if (r1 == 0 && r2 == 0) { r = phi = 0; }
    else if (r1 * r1 > r2 * r2) { r = r1; phi = (float)((kPi / 4.0f) * (r2 / r1)); }
    else { r = r2; phi = (float)((kPi / 2.0f) - (r1 / r2) * (kPi / 4.0f)); }
    const float px = r * (float)cos((double)phi), py = r * (float)sin((double)phi);
    float z = safe_sqrt(1.0f - px * px - py * py);
    if (z == 0) z = 1e-10f;
    return f3(px, py, z);
}

__device__ void frame_of(F3 a, F3* b, F3* c)   // coordinateSystem, util.cpp:592-601
{
    if (fabsf(a.x) > fabsf(a.y)) {
        const float invLen = 1.0f / sqrtf(a.x * a.x + a.z * a.z);
        *c = f3(a.z * invLen, 0.0f, -a.x * invLen);
    } else {
        const float invLen = 1.0f / sqrtf(a.y * a.y + a.z * a.z);
        *c = f3(0.0f, a.z * invLen, -a.y * invLen);
    }
    *b = cross(*c, a);
}

__device__ float box_hit(const TScene& sc, F3 o, F3 d, F3* n)   // first wall hit from inside
{
    float best = INFINITY;
    int axis = -1;
    const float oo[3] = {o.x, o.y, o.z}, dd[3] = {d.x, d.y, d.z};
    for (int a = 0; a < 3; a++) {
        float t;
        if (dd[a] > 0) t = (sc.box_max[a] - oo[a]) / dd[a];
        else if (dd[a] < 0) t = (sc.box_min[a] - oo[a]) / dd[a];
        else continue;
        if (t < best) { best = t; axis = a; }
    }
    float nn[3] = {0.0f, 0.0f, 0.0f};
    if (axis >= 0) nn[axis] = dd[axis] > 0 ? -1.0f : 1.0f;
    *n = f3(nn[0], nn[1], nn[2]);
    return best;
}

// Scene::rayIntersect over the walls and the occluders (host SmokeBox::first_hit):
// t, normal, its.p (ray(t) on a wall, barycentric on a triangle), occluder or not
// *tri: the occluder's index (-1: a wall)
__device__ float first_hit(const TScene& sc, F3 o, F3 d, float mint, F3* n, F3* p, int* tri)
{
    float best = box_hit(sc, o, d, n);
    int id = -1, slot = -1;
    float bu = 0.0f, bv = 0.0f;
    alvrl::bvh::closest(sc.bv, alvrl::bvh::mk(o.x, o.y, o.z), alvrl::bvh::mk(d.x, d.y, d.z), mint, &best, &id, &slot,
                        &bu, &bv);
    *tri = id;
    if (id < 0) {
        *p = add(o, mul(d, best));
        return best;
    }
    const float* q = sc.bv.tris + 9 * (size_t)slot;
    const F3 p0 = f3(q[0], q[1], q[2]), p1 = f3(q[3], q[4], q[5]), p2 = f3(q[6], q[7], q[8]);
    const float b0 = 1 - bu - bv;
    *p = add(add(mul(p0, b0), mul(p1, bu)), mul(p2, bv));
    F3 fn = cross(sub(p1, p0), sub(p2, p0));
    const float l = len(fn);
    if (!(fn.x == 0 && fn.y == 0 && fn.z == 0)) fn = mul(fn, 1.0f / l);
    *n = fn;
    return best;
}

// the diffuse reflectance of what first_hit hit: the occluder's own or the shared one, or the walls'
__device__ __forceinline__ const float* albedo_of(const TScene& sc, int tri)
{
    return tri < 0 ? sc.albedo : sc.occ_alb ? sc.occ_alb + 3 * (size_t)tri : sc.occ_albedo;
}

// the BSDF of what first_hit hit (SmokeBox::mat): 0 diffuse (the walls too), 1 mirror, 2 null, 3 dielectric
__device__ __forceinline__ uint32_t mat_of(const TScene& sc, int tri)
{
    return (tri < 0 || !sc.occ_mat) ? 0u : sc.occ_mat[(size_t)tri];
}

// fresnelDielectricExt (util.cpp:651-681), the host's fresnel_dielectric_ext operation for operation
__device__ float fresnel_dielectric_ext(float cos_theta_i, float* cos_theta_t, float eta)
{
    if (eta == 1) {
        *cos_theta_t = -cos_theta_i;
        return 0.0f;
    }
    const float scale = (cos_theta_i > 0) ? 1 / eta : eta;
    const float cos_t_sqr = 1 - (1 - cos_theta_i * cos_theta_i) * (scale * scale);
    if (cos_t_sqr <= 0.0f) {   // total internal reflection
        *cos_theta_t = 0.0f;
        return 1.0f;
    }
    const float ci = fabsf(cos_theta_i);
    const float ct = sqrtf(cos_t_sqr);
    const float Rs = (ci - eta * ct) / (ci + eta * ct);
    const float Rp = (eta * ci - ct) / (eta * ci + ct);
    *cos_theta_t = (cos_theta_i > 0) ? -ct : ct;
    return 0.5f * (Rs * Rs + Rp * Rp);
}

// vrlVector::put + the current VRL (vrlTracer.h:56-89, VRL.h:148-158); counts,
// or writes into the SoA planes at 'pos' when soa != nullptr
struct Sink {
    F3 start;
    float power[3];
    int sigma_s_zero;
    uint32_t n;
    float* soa;
    uint64_t pos, stride;
    __device__ void put(F3 end)
    {
        if (sigma_s_zero) return;
        if (power[0] == 0 && power[1] == 0 && power[2] == 0) return;
        if (len(sub(start, end)) == 0) return;
        if (soa) {
            const uint64_t i = pos + n;
            const float v[9] = {start.x, start.y, start.z, end.x, end.y, end.z, power[0], power[1], power[2]};
#pragma unroll
            for (int pl = 0; pl < 9; pl++) soa[(uint64_t)pl * stride + i] = v[pl];
        }
        n++;
    }
    __device__ void end_current(F3 p)
    {
        if (len(sub(start, p)) == 0) return;
        put(p);
    }
};

// SmokeBox::sample_area_emission (host/scene.cpp), the same operations:
// Scene::sampleEmitterPosition with one emitter, TriMesh::samplePosition,
// Triangle::sample, AreaEmitter::sampleDirection (area.cpp:94-123)
__device__ F3 area_emission(const TScene& sc, float sx, float sy, float dx, float dy, F3* dir, float power[3])
{
    const uint32_t n = sc.nemit;
    uint32_t lb = 0;
    while (lb <= n && sc.emit_cdf[lb] < sy) lb++;   // std::lower_bound
    uint32_t idx = lb > 0 ? lb - 1 : 0;
    if (idx > n - 1) idx = n - 1;
    while (idx + 1 < n && sc.emit_cdf[idx + 1] - sc.emit_cdf[idx] == 0) ++idx;
    const float y = (sy - sc.emit_cdf[idx]) / (sc.emit_cdf[idx + 1] - sc.emit_cdf[idx]);
    const float a = safe_sqrt(1.0f - sx);
    const float bx = 1 - a, by = a * y;
    const float* t = sc.emit + 9 * (size_t)idx;
    const F3 p0 = f3(t[0], t[1], t[2]);
    const F3 sideA = sub(f3(t[3], t[4], t[5]), p0), sideB = sub(f3(t[6], t[7], t[8]), p0);
    const F3 o = add(add(p0, mul(sideA, bx)), mul(sideB, by));
    const F3 c = cross(sideA, sideB);
    const F3 nn = mul(c, 1.0f / len(c));
    for (int i = 0; i < 3; i++) power[i] = (sc.emit_radiance[i] * (float)kPi) * sc.emit_area;
    const F3 l = cosine_hemisphere(dx, dy);
    F3 fs, ft;
    frame_of(nn, &fs, &ft);
    *dir = add(add(mul(fs, l.x), mul(ft, l.y)), mul(nn, l.z));
    return o;
}

__device__ void trace_particle(const TScene& sc, Stream& smp, bool short_vrls, int max_depth, int rr_depth, Sink& k)
{
    const float sx = smp.next(), sy = smp.next();   // sampleEmitterPosition (scene.cpp:958-974)
    const float dx = smp.next(), dy = smp.next();   // sampleDirection (point.cpp:99-106, area.cpp:115-123)
    float power[3];
    F3 dir, o;
    if (sc.nemit) {
        o = area_emission(sc, sx, sy, dx, dy, &dir, power);
    } else {
        dir = uniform_sphere(dx, dy);
        o = f3(sc.light_pos[0], sc.light_pos[1], sc.light_pos[2]);
        for (int i = 0; i < 3; i++) power[i] = sc.power[i];
    }
    if (power[0] == 0 && power[1] == 0 && power[2] == 0) return;
    k.start = o;
    for (int i = 0; i < 3; i++) k.power[i] = power[i];
    int depth = 1;
    float thr[3] = {1.0f, 1.0f, 1.0f};
    float eta = 1.0f;
    float mint = 1e-4f;   // Ray() default mint (Epsilon), then 0 after a medium and Epsilon after a surface
    // bounded like the host's loop: max_depth when set, else the roulette from
    // rr_depth on (survival <= 0.95 per iteration) and the throughput reaching 0
    while (!(thr[0] == 0 && thr[1] == 0 && thr[2] == 0) && (depth <= max_depth || max_depth < 0)) {
        F3 n, hp;
        int hit_tri;
        const float its_t = first_hit(sc, o, dir, mint, &n, &hp, &hit_tri);
        const bool its_valid = isfinite(its_t);
        // HomogeneousMedium::sampleDistance (homogeneous.cpp:275-352), balance
        float pdf_max = 0.0f;
        float sampled = sample_distance(sc, smp, &pdf_max);
        const float distSurf = its_t - 0.0f;
        bool success = true;
        F3 mp = o;
        if (sampled < distSurf) {
            mp = add(o, mul(dir, sampled + 0.0f));
            if (mp.x == o.x && mp.y == o.y && mp.z == o.z) success = false;
        } else {
            sampled = distSurf;
            success = false;
        }
        float pf, ps;
        medium_pdfs(sc, sampled, pdf_max, &ps, &pf);
        float mtr[3];
        for (int i = 0; i < 3; i++) mtr[i] = fastexp(sc.sigma_t[i] * (-sampled));
        {
            float mx = mtr[0] > mtr[1] ? mtr[0] : mtr[1];
            mx = mx > mtr[2] ? mx : mtr[2];
            if (mx < 1e-20f) mtr[0] = mtr[1] = mtr[2] = 0;
        }
        if (success) {   // vrlTracer.h:143-172
            const float rps = 1.0f / ps;
            for (int i = 0; i < 3; i++) thr[i] *= mtr[i] * sc.sigma_s[i] * rps;
            const float px_ = smp.next(), py_ = smp.next();
            const F3 wo = uniform_sphere(px_, py_);
            const F3 endPoint = short_vrls ? mp : hp;
            k.end_current(endPoint);
            k.start = mp;
            for (int i = 0; i < 3; i++) k.power[i] = thr[i] * power[i];
            o = mp; dir = wo; mint = 0.0f;
        } else if (its_valid) {   // vrlTracer.h:173-213
            const float rpf = 1.0f / pf;
            for (int i = 0; i < 3; i++) thr[i] *= mtr[i] * rpf;
            const F3 p = hp;
            const float* alb = albedo_of(sc, hit_tri);
            F3 fs, ft;
            frame_of(n, &fs, &ft);
            const F3 mwi = f3(-dir.x, -dir.y, -dir.z);
            const float cos_wi = dot(mwi, n);
            const float bx = smp.next(), by = smp.next();
            float bw[3] = {0, 0, 0};
            F3 wol = f3(0, 0, 0);
            const uint32_t mt = mat_of(sc, hit_tri);
            if (mt == 0u) {          // SmoothDiffuse::sample (diffuse.cpp:120-133)
                if (!(cos_wi <= 0)) {
                    wol = cosine_hemisphere(bx, by);
                    for (int i = 0; i < 3; i++) bw[i] = alb[i];
                }
            } else if (mt == 1u) {   // SmoothConductor::sample (conductor.cpp:254-268), material none
                if (!(cos_wi <= 0)) {
                    wol = f3(-dot(mwi, fs), -dot(mwi, ft), cos_wi);   // reflect(wi)
                    for (int i = 0; i < 3; i++) bw[i] = sc.occ_spec[i];
                }
            } else if (mt == 3u) {   // SmoothDielectric::sample, both components, EImportance (dielectric.cpp:335-364)
                float cos_t;
                const float F = fresnel_dielectric_ext(cos_wi, &cos_t, sc.occ_eta);
                if (bx <= F) {
                    wol = f3(-dot(mwi, fs), -dot(mwi, ft), cos_wi);
                } else {
                    const float inv_eta = 1 / sc.occ_eta;
                    const float scale = -(cos_t < 0 ? inv_eta : sc.occ_eta);   // refract(wi, cosThetaT)
                    wol = f3(scale * dot(mwi, fs), scale * dot(mwi, ft), cos_t);
                    eta *= cos_t < 0 ? sc.occ_eta : inv_eta;                   // bRec.eta
                }
                bw[0] = bw[1] = bw[2] = 1.0f;                                 // importance: factor 1
            } else {                 // Null::sample (null.cpp:53-63): wo = -wi
                wol = f3(-dot(mwi, fs), -dot(mwi, ft), -cos_wi);
                bw[0] = bw[1] = bw[2] = 1.0f;
            }
            if (bw[0] == 0 && bw[1] == 0 && bw[2] == 0) { k.end_current(p); break; }
            const F3 wo = add(add(mul(fs, wol.x), mul(ft, wol.y)), mul(n, wol.z));
            const float wiDotGeoN = dot(n, mwi), woDotGeoN = dot(n, wo);
            if (wiDotGeoN * cos_wi <= 0 || woDotGeoN * wol.z <= 0) { k.end_current(p); break; }
            for (int i = 0; i < 3; i++) thr[i] *= bw[i];
            k.end_current(p);
            k.start = p;
            for (int i = 0; i < 3; i++) k.power[i] = thr[i] * power[i];
            o = p; dir = wo; mint = 1e-4f;
        } else {
            break;
        }
        if (depth++ >= rr_depth) {
            float mx = thr[0] > thr[1] ? thr[0] : thr[1];
            mx = mx > thr[2] ? mx : thr[2];
            float q = mx * eta * eta;
            if (q > 0.95f) q = 0.95f;
            if (smp.next() >= q) break;
            const float rq = 1.0f / q;
            for (int i = 0; i < 3; i++) thr[i] *= rq;
        }
    }
}

struct TArgs {
    uint32_t seed, pass;
    int short_vrls, max_depth, rr_depth;
};

__global__ void __launch_bounds__(256) k_trace_count(TScene sc, TArgs a, uint64_t p0, uint32_t P, uint32_t* counts)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= P) return;
    const uint64_t p = p0 + i;
    Stream smp{a.seed, a.pass, (uint32_t)p, (uint32_t)(p >> 32), 0u, 0xFFFFFFFFu, {0, 0, 0, 0}};
    Sink k{};
    k.sigma_s_zero = sc.sigma_s_zero;
    k.soa = nullptr;
    trace_particle(sc, smp, a.short_vrls != 0, a.max_depth, a.rr_depth, k);
    counts[i] = k.n;
}

__global__ void __launch_bounds__(256) k_trace_write(TScene sc, TArgs a, uint64_t p0, uint32_t P,
                                                     const uint64_t* offs, float* soa, uint64_t stride)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= P) return;
    const uint64_t p = p0 + i;
    Stream smp{a.seed, a.pass, (uint32_t)p, (uint32_t)(p >> 32), 0u, 0xFFFFFFFFu, {0, 0, 0, 0}};
    Sink k{};
    k.sigma_s_zero = sc.sigma_s_zero;
    k.soa = soa;
    k.pos = offs[i];
    k.stride = stride;
    trace_particle(sc, smp, a.short_vrls != 0, a.max_depth, a.rr_depth, k);
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

// The camera of SmokeBox::camera_ray with its per-scene terms formed on the
// host (the same float operations, so the same values).
struct TCam {
    float o[3], fwd[3], left[3], nup[3];
    float tanh_, aspect, inv_w, inv_h;
    uint32_t width;
    int scat;
};

// Sensor::sampleRay at the pixel centre + Scene::rayIntersect (host
// SmokeBox::make_record, bit for bit): the GPU eye-ray first hit of SURVEY
// 8(f) row 1.  pix == nullptr: pixel i.
// Sensor sample j of spp > 1 (SmokeBox::pixel_sample): draws 0 and 1 of the
// counter stream (seed, pass, dom 8, pixel, j).
constexpr uint32_t kDomPixel = 8u;
__device__ __forceinline__ void pixel_jitter(uint32_t seed, uint32_t pass, uint32_t pixel, uint32_t j, float* u,
                                             float* v)
{
    uint32_t c0 = pixel, c1 = j, c2 = 0u, c3 = kDomPixel << 24;
    uint32_t k0 = seed, k1 = pass;
    for (int r = 0; r < 10; r++) {
        if (r > 0) { k0 += 0x9E3779B9u; k1 += 0xBB67AE85u; }
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c0 = n0; c1 = (uint32_t)p1; c2 = n2; c3 = (uint32_t)p0;
    }
    *u = __uint_as_float((c0 >> 9) | 0x3f800000u) - 1.0f;
    *v = __uint_as_float((c1 >> 9) | 0x3f800000u) - 1.0f;
}

// Sensor::sampleRay through sensor sample j of spp of pixel id (SmokeBox::pixel_sample + camera_ray)
__device__ __forceinline__ void sensor_ray(const TCam& c, uint32_t id, uint32_t j, uint32_t spp, uint32_t seed,
                                           uint32_t pass, F3* O, F3* D, float* mint)
{
    float px = (float)(id % c.width) + 0.5f, py = (float)(id / c.width) + 0.5f;
    if (spp > 1) {
        float u, v;
        pixel_jitter(seed, pass, id, j, &u, &v);
        px = (float)(id % c.width) + u;
        py = (float)(id / c.width) + v;
    }
    const float sx = px * c.inv_w, sy = py * c.inv_h;
    const float xc = (1.0f - 2.0f * sx) * c.tanh_;
    const float yc = ((1.0f - 2.0f * sy) / c.aspect) * c.tanh_;
    F3 dc = f3(xc, yc, 1.0f);
    dc = mul(dc, 1.0f / len(dc));
    *mint = 1e-2f * (1.0f / dc.z);
    *O = f3(c.o[0], c.o[1], c.o[2]);
    *D = f3(c.left[0] * dc.x + c.nup[0] * dc.y + c.fwd[0] * dc.z,
            c.left[1] * dc.x + c.nup[1] * dc.y + c.fwd[1] * dc.z,
            c.left[2] * dc.x + c.nup[2] * dc.y + c.fwd[2] * dc.z);
}

// spp records per pixel, sample major: record j * n + i is pixel pix[i],
// sensor sample j (its depth word j << 16); spp == 1: pixel centres.
__global__ void __launch_bounds__(256) k_eye_records(TCam c, TScene sc, const uint32_t* __restrict__ pix,
                                                     uint32_t n, uint32_t spp, uint32_t seed, uint32_t pass,
                                                     float* __restrict__ out)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n * spp) return;
    const uint32_t j = i / n, ii = i - j * n;
    const uint32_t id = pix ? pix[ii] : ii;
    F3 O, D;
    float mint;
    sensor_ray(c, id, j, spp, seed, pass, &O, &D, &mint);
    F3 nn, p;
    int tri;
    const float t = first_hit(sc, O, D, mint, &nn, &p, &tri);
    const uint32_t m = mat_of(sc, tri);
    uint32_t flags = 0;
    if (isfinite(t)) flags |= 1u | (m == 0u ? 2u : 8u);   // ESmooth (diffuse) or EDelta, as SmokeBox::make_record
    if (c.scat) flags |= 4u;
    const float* a = albedo_of(sc, tri);
    float* r = out + 20 * (size_t)i;   // alvrl_gather_rec: 20 words
    const float v[15] = {O.x, O.y, O.z, D.x, D.y, D.z, p.x, p.y, p.z, nn.x, nn.y, nn.z,
                         m == 0u ? a[0] : 0.0f, m == 0u ? a[1] : 0.0f, m == 0u ? a[2] : 0.0f};
#pragma unroll
    for (int k = 0; k < 15; k++) r[k] = v[k];
    r[15] = __uint_as_float(flags);
    r[16] = 1.0f; r[17] = 1.0f; r[18] = 1.0f;   // a camera ray: path weight 1, depth 0
    r[19] = __uint_as_float(j << 16);
}

// ------------------------------------------------------ eye-path chains --
// SmokeBox::chain_node (host/scene.cpp), LiInternal's recursion through delta
// BSDFs (vrlIntegrator.cpp:398-524), as an explicit pre-order traversal: one
// lane per pixel.  A node is one LiInternal call: the record of the ray's
// hit, then each delta component's continuation.  The roulette stream of a
// node is keyed by the node's own record index (seed, pass, dom 7, pixel,
// k | sample << 16) and only that node draws from it, in component order, so
// both children are decided when the node is visited: the lane goes on with
// the first surviving child and, at a dielectric whose reflection and
// refraction both survive, parks the refracted one on its pending-sibling
// stack until the reflected subtree is finished -- the host's depth-first
// order, which fixes every record's index.
constexpr uint32_t kDomEye = 7u;
constexpr uint32_t kChainMaxRecs = 256u;     // SmokeBox::chain_node's cap
constexpr uint32_t kChainStackDefault = 8u;  // pending siblings per lane
constexpr uint32_t kChainStackMax = 255u;    // a sibling is parked by a node that wrote a record
constexpr uint32_t kChainOverflow = 0xFFFFFFFFu;   // the count of a pixel whose tree needs a deeper stack
constexpr int kChainNodeWords = 13;          // p, direction, path weight, throughput, depth

struct CArgs {
    uint32_t seed, pass, sample, spp, flags, cap;   // flags: HIT | MEDIUM of every record; cap: stack entries per lane
    int spec_rr_depth;
    float init_thr;
};

struct CNode {
    F3 o, d;
    float w[3], thr[3];
    int depth;
};

// draws 0 and 1 of the node's roulette stream (the host's Stream{seed, pass, kDomEye, pixel, kw, 0})
__device__ __forceinline__ void eye_draws(uint32_t seed, uint32_t pass, uint32_t pixel, uint32_t kw, float u[2])
{
    uint32_t c0 = pixel, c1 = kw, c2 = 0u, c3 = kDomEye << 24;
    uint32_t k0 = seed, k1 = pass;
    for (int r = 0; r < 10; r++) {
        if (r > 0) { k0 += 0x9E3779B9u; k1 += 0xBB67AE85u; }
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c0 = n0; c1 = (uint32_t)p1; c2 = n2; c3 = (uint32_t)p0;
    }
    u[0] = __uint_as_float((c0 >> 9) | 0x3f800000u) - 1.0f;
    u[1] = __uint_as_float((c1 >> 9) | 0x3f800000u) - 1.0f;
}

// The pending siblings of lane 'lane' of 'lanes': word w of entry e at
// stack[(e * kChainNodeWords + w) * lanes + lane], so a wave's pushes coalesce.
__device__ __forceinline__ void chain_push(float* stack, uint64_t lanes, uint64_t lane, uint32_t e, const CNode& nd)
{
    const float v[kChainNodeWords] = {nd.o.x, nd.o.y, nd.o.z, nd.d.x, nd.d.y, nd.d.z, nd.w[0], nd.w[1], nd.w[2],
                                      nd.thr[0], nd.thr[1], nd.thr[2], __int_as_float(nd.depth)};
#pragma unroll
    for (int w = 0; w < kChainNodeWords; w++) stack[((uint64_t)e * kChainNodeWords + w) * lanes + lane] = v[w];
}

__device__ __forceinline__ CNode chain_pop(const float* stack, uint64_t lanes, uint64_t lane, uint32_t e)
{
    float v[kChainNodeWords];
#pragma unroll
    for (int w = 0; w < kChainNodeWords; w++) v[w] = stack[((uint64_t)e * kChainNodeWords + w) * lanes + lane];
    CNode nd;
    nd.o = f3(v[0], v[1], v[2]); nd.d = f3(v[3], v[4], v[5]);
    for (int i = 0; i < 3; i++) { nd.w[i] = v[6 + i]; nd.thr[i] = v[9 + i]; }
    nd.depth = __float_as_int(v[12]);
    return nd;
}

// The eye path of pixel 'pixel' from the sensor ray (O, D, mint).  Returns the
// number of records (record 0 is the primary record, which k_eye_records
// writes), or kChainOverflow when the pending siblings exceed a.cap.  With
// out != nullptr record k >= 1 goes to out[pos[k - 1]] and its source index
// to src[pos[k - 1]], for k < limit only (the pixel's count from the count
// pass: the write pass never leaves the pixel's offsets).
__device__ uint32_t chain_walk(const TScene& sc, const CArgs& a, uint32_t pixel, F3 O, F3 D, float mint0, float* stack,
                               uint64_t lanes, uint64_t lane, float* out, uint32_t* src, const uint32_t* pos,
                               uint32_t limit, uint32_t src_index)
{
    CNode cur;
    cur.o = O; cur.d = D;
    for (int i = 0; i < 3; i++) { cur.w[i] = 1.0f; cur.thr[i] = a.init_thr; }   // throughputWithEtaSq (:381)
    cur.depth = 1;
    float mint = mint0;
    uint32_t k = 0, sp = 0;
    // One iteration per visited node.  Bound: a node either writes a record
    // (at most kChainMaxRecs of them: the loop ends at k == 256, where the
    // host's remaining calls all return at once) or ends its branch and pops
    // a sibling (at most one per record written), so <= 512 iterations.
    while (k < kChainMaxRecs) {
        bool alive = false;
        CNode next;
        F3 n, p;
        int tri;
        const float t = first_hit(sc, cur.o, cur.d, mint, &n, &p, &tri);
        if (isfinite(t)) {                                                   // :414-419
            const uint32_t m = mat_of(sc, tri);
            const uint32_t kw = k | (a.sample << 16);
            if (out && k >= 1 && k < limit) {
                const float* al = albedo_of(sc, tri);
                float* r = out + 20 * (size_t)pos[k - 1];
                const float v[15] = {cur.o.x, cur.o.y, cur.o.z, cur.d.x, cur.d.y, cur.d.z, p.x, p.y, p.z, n.x, n.y, n.z,
                                     m == 0u ? al[0] : 0.0f, m == 0u ? al[1] : 0.0f, m == 0u ? al[2] : 0.0f};
#pragma unroll
                for (int q = 0; q < 15; q++) r[q] = v[q];
                r[15] = __uint_as_float(a.flags | (m == 0u ? 2u : 8u));
                r[16] = cur.w[0]; r[17] = cur.w[1]; r[18] = cur.w[2];
                r[19] = __uint_as_float(kw);
                src[pos[k - 1]] = src_index;
            }
            ++k;
            float tr[3] = {0.0f, 0.0f, 0.0f};
            if (m != 0u) {   // the segment's transmittance (:450-460); a diffuse hit has no delta component (:447-448)
                for (int i = 0; i < 3; i++) tr[i] = fastexp(sc.sigma_t[i] * (-t));
                float mx = tr[0] > tr[1] ? tr[0] : tr[1];
                mx = mx > tr[2] ? mx : tr[2];
                if (mx < 1e-20f) tr[0] = tr[1] = tr[2] = 0;
            }
            if (!(tr[0] == 0 && tr[1] == 0 && tr[2] == 0)) {
                F3 fs, ft;
                frame_of(n, &fs, &ft);
                const F3 mwi = f3(-cur.d.x, -cur.d.y, -cur.d.z);
                const float cos_wi = dot(mwi, n);
                float u[2] = {0.0f, 0.0f};
                bool drawn = false;
                int nd = 0;   // draws taken from this node's stream
                const int ncomp = m == 3u ? 2 : 1;
                CNode child[2];
                bool live[2] = {false, false};
                // the delta components (:467-511): at most 2
                for (int c = 0; c < ncomp; c++) {
                    float bw[3];
                    float beta = 1.0f;   // bRec.eta
                    F3 wol;
                    if (m == 1u) {          // conductor.cpp:254-268
                        if (cos_wi <= 0) continue;
                        wol = f3(-dot(mwi, fs), -dot(mwi, ft), cos_wi);
                        for (int i = 0; i < 3; i++) bw[i] = sc.occ_spec[i];
                    } else if (m == 2u) {   // null.cpp:53-63
                        wol = f3(-dot(mwi, fs), -dot(mwi, ft), -cos_wi);
                        bw[0] = bw[1] = bw[2] = 1.0f;
                    } else {                // dielectric.cpp:365-385, one component, ERadiance
                        float cos_t;
                        const float F = fresnel_dielectric_ext(cos_wi, &cos_t, sc.occ_eta);
                        const float inv_eta = 1 / sc.occ_eta;
                        if (c == 0) {
                            wol = f3(-dot(mwi, fs), -dot(mwi, ft), cos_wi);
                            bw[0] = bw[1] = bw[2] = F;
                        } else {
                            const float scale = -(cos_t < 0 ? inv_eta : sc.occ_eta);
                            wol = f3(scale * dot(mwi, fs), scale * dot(mwi, ft), cos_t);
                            beta = cos_t < 0 ? sc.occ_eta : inv_eta;
                            const float factor = cos_t < 0 ? inv_eta : sc.occ_eta;
                            bw[0] = bw[1] = bw[2] = factor * factor * (1 - F);
                        }
                        if (bw[0] == 0) continue;
                    }
                    // Russian roulette (:480-492)
                    float thr2[3];
                    for (int i = 0; i < 3; i++) thr2[i] = ((cur.thr[i] * tr[i]) * bw[i]) * (beta * beta);
                    const float maxRR = cur.depth >= a.spec_rr_depth ? 0.98f : 1.0f;
                    float mx = thr2[0] > thr2[1] ? thr2[0] : thr2[1];
                    mx = mx > thr2[2] ? mx : thr2[2];
                    const float rrProb = maxRR < mx ? maxRR : mx;
                    if (rrProb <= 0) continue;
                    if (rrProb < 1) {
                        if (!drawn) { eye_draws(a.seed, a.pass, pixel, kw, u); drawn = true; }
                        if (u[nd++] > rrProb) continue;
                    }
                    CNode& ch = child[c];
                    for (int i = 0; i < 3; i++) {
                        ch.thr[i] = thr2[i] / rrProb;
                        ch.w[i] = ((cur.w[i] * tr[i]) * bw[i]) / rrProb;   // weight * transmittance * bsdfWeight / rrProb (:505)
                    }
                    ch.o = p;
                    ch.d = add(add(mul(fs, wol.x), mul(ft, wol.y)), mul(n, wol.z));   // its.toWorld(bRec.wo)
                    ch.depth = cur.depth + 1;
                    live[c] = true;
                }
                if (live[0] && live[1]) {
                    if (sp >= a.cap) return kChainOverflow;   // the entry point completes this pixel on the host
                    chain_push(stack, lanes, lane, sp++, child[1]);
                }
                if (live[0]) { next = child[0]; alive = true; }
                else if (live[1]) { next = child[1]; alive = true; }
            }
        }
        if (!alive) {
            if (sp == 0) break;
            next = chain_pop(stack, lanes, lane, --sp);
        }
        cur = next;
        mint = 1e-4f;   // RayDifferential(its.p, wo): mint = Epsilon
    }
    return k;
}

// count pass: counts[i] = records of pixel i's eye path (kChainOverflow: its
// index is appended to ovf, *n_ovf counting them; at most n)
// One launch covers pixels i0 .. i0 + lanes - 1 (those below n); the stack
// workspace holds 'lanes' lanes.
__global__ void __launch_bounds__(256) k_chain_count(TCam c, TScene sc, CArgs a, const uint32_t* __restrict__ pix,
                                                     uint32_t i0, uint32_t lanes, uint32_t n,
                                                     float* __restrict__ stack, uint32_t* __restrict__ counts,
                                                     uint32_t* __restrict__ ovf, uint32_t* __restrict__ n_ovf)
{
    const uint32_t lane = blockIdx.x * blockDim.x + threadIdx.x;
    if (lane >= lanes || lane >= n - i0) return;
    const uint32_t i = i0 + lane;
    const uint32_t id = pix ? pix[i] : i;
    F3 O, D;
    float mint;
    sensor_ray(c, id, a.sample, a.spp, a.seed, a.pass, &O, &D, &mint);
    const uint32_t k = chain_walk(sc, a, id, O, D, mint, stack, lanes, lane, nullptr, nullptr, nullptr, 0u, i);
    counts[i] = k;
    if (k == kChainOverflow) {
        const uint32_t slot = atomicAdd(n_ovf, 1u);
        if (slot < n) ovf[slot] = i;
    }
}

// write pass: pixel i's records 1..counts[i]-1 at the positions pos[base[i]..]
// the entry point derived from the counts; an overflowed pixel is the host's
__global__ void __launch_bounds__(256) k_chain_write(TCam c, TScene sc, CArgs a, const uint32_t* __restrict__ pix,
                                                     uint32_t i0, uint32_t lanes, uint32_t n,
                                                     float* __restrict__ stack,
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
    const uint32_t id = pix ? pix[i] : i;
    F3 O, D;
    float mint;
    sensor_ray(c, id, a.sample, a.spp, a.seed, a.pass, &O, &D, &mint);
    (void)chain_walk(sc, a, id, O, D, mint, stack, lanes, lane, out, src, pos + base[i], cnt, i);
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
constexpr uint32_t kDomVolpath = 6u;

struct VStream {
    uint32_t seed, pass, a, b, k, blk;
    uint32_t buf[4];
    __device__ float next()
    {
        const uint32_t bl = k >> 2;
        if (bl != blk) {
            uint32_t c0 = a, c1 = b, c2 = bl, c3 = (kDomVolpath << 24);
            uint32_t k0 = seed, k1 = pass;
            for (int r = 0; r < 10; r++) {
                if (r > 0) { k0 += 0x9E3779B9u; k1 += 0xBB67AE85u; }
                const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
                const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
                c0 = n0; c1 = (uint32_t)p1; c2 = n2; c3 = (uint32_t)p0;
            }
            buf[0] = c0; buf[1] = c1; buf[2] = c2; buf[3] = c3;
            blk = bl;
        }
        const uint32_t u = (buf[k & 3] >> 9) | 0x3f800000u;
        ++k;
        return __uint_as_float(u) - 1.0f;
    }
};

struct VParams {
    int max_depth, rr_depth, only_vrl, vol_to_vol, vol_to_surf;
    float intensity[3];
};

// evalTransmittance(p1, p1OnSurface, light, false) (scene.cpp:619-679):
// medium transmittance over the whole segment, 0 behind an occluder
__device__ void attenuation(const TScene& sc, F3 p1, bool p1_surface, F3 p2, float tr[3])
{
    const F3 d0 = sub(p2, p1);
    const float remaining = len(d0);
    const float negLength = 0.0f - remaining;
    for (int i = 0; i < 3; i++) tr[i] = sc.sigma_t[i] != 0 ? fastexp(sc.sigma_t[i] * negLength) : 1.0f;
    if (sc.bv.ntri && remaining > 0) {
        const F3 d = mul(d0, 1.0f / remaining);
        if (alvrl::bvh::occluded(sc.bv, alvrl::bvh::mk(p1.x, p1.y, p1.z), alvrl::bvh::mk(d.x, d.y, d.z),
                                 p1_surface ? 1e-4f : 0.0f, remaining))
            tr[0] = tr[1] = tr[2] = 0.0f;
    }
}

// Scene::sampleAttenuatedEmitterDirect + PointEmitter::sampleDirect
// (scene.cpp:854-898, point.cpp:131-147): value and unit direction to the light
__device__ void light_direct(const TScene& sc, const VParams& vp, F3 ref, bool on_surface, float val[3], F3* dir)
{
    const F3 L = f3(sc.light_pos[0], sc.light_pos[1], sc.light_pos[2]);
    F3 d = sub(L, ref);
    const float dist = len(d);
    const float invDist = 1.0f / dist;
    d = mul(d, invDist);
    *dir = d;
    float tr[3];
    attenuation(sc, ref, on_surface, L, tr);
    for (int i = 0; i < 3; i++) {
        val[i] = vp.intensity[i] * (invDist * invDist);
        val[i] *= tr[i] * 1.0f;   // / emPdf (one emitter)
    }
}

__device__ void volpath_li(const TScene& sc, const VParams& vp, VStream& smp, F3 o, F3 dir, float mint, float Li[3])
{
    Li[0] = Li[1] = Li[2] = 0.0f;
    bool first_ok = false, second_ok = false, prev_diffuse = false, prev_volume = false;
    F3 n, hp;
    int hit_tri;
    float its_t = first_hit(sc, o, dir, mint, &n, &hp, &hit_tri);
    float thr[3] = {1.0f, 1.0f, 1.0f};
    const float eta = 1.0f;
    int depth = 1;
    bool indirect = true;   // rRec.type keeps EIndirect*Radiance (ERadiance / ERadianceNoEmission)
    while (depth <= vp.max_depth || vp.max_depth < 0) {
        if (vp.only_vrl && depth > 2 && !(first_ok && second_ok)) break;   // :144-145
        // HomogeneousMedium::sampleDistance over Ray(ray, 0, its.t)
        float pdf_max = 0.0f;
        float sampled = sample_distance(sc, smp, &pdf_max);
        const float distSurf = its_t - 0.0f;
        bool success = true;
        F3 mp = o;
        if (sampled < distSurf) {
            mp = add(o, mul(dir, sampled + 0.0f));
            if (mp.x == o.x && mp.y == o.y && mp.z == o.z) success = false;
        } else {
            sampled = distSurf;
            success = false;
        }
        float pf, ps;
        medium_pdfs(sc, sampled, pdf_max, &ps, &pf);
        float mtr[3];
        for (int i = 0; i < 3; i++) mtr[i] = fastexp(sc.sigma_t[i] * (-sampled));
        {
            float mx = mtr[0] > mtr[1] ? mtr[0] : mtr[1];
            mx = mx > mtr[2] ? mx : mtr[2];
            if (mx < 1e-20f) mtr[0] = mtr[1] = mtr[2] = 0;
        }
        if (success) {   // :150-267
            if (depth == 1 && vp.vol_to_vol) first_ok = true;
            if (depth == 2) second_ok = true;
            if (depth >= vp.max_depth && vp.max_depth != -1) break;
            const float rps = 1.0f / ps;
            for (int i = 0; i < 3; i++) thr[i] *= (sc.sigma_s[i] * mtr[i]) * rps;
            // luminaire sampling; the reference's "(!rRec.depth==2 || ...)" is
            // "((!depth) == 2 || ...)", i.e. the bracket alone (:183-190)
            const bool nee = !vp.only_vrl ||
                             (depth != 1 && (prev_volume || prev_diffuse) && (!prev_diffuse || vp.vol_to_surf) &&
                              (!prev_volume || vp.vol_to_vol));
            if (nee) {
                (void)smp.next(); (void)smp.next();   // rRec.nextSample2D() (unused by a point light)
                float val[3];
                F3 ld;
                light_direct(sc, vp, mp, false, val, &ld);
                if (!(val[0] == 0 && val[1] == 0 && val[2] == 0)) {
                    const float phaseVal = 0.079577471545947667884f;   // IsotropicPhaseFunction::eval, 1/(4 pi)
                    for (int i = 0; i < 3; i++) Li[i] += ((thr[i] * val[i]) * phaseVal) * 1.0f;
                }
            }
            // phase sampling (isotropic: weight 1)
            const float px_ = smp.next(), py_ = smp.next();
            const F3 wo = uniform_sphere(px_, py_);
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
            const float* alb = albedo_of(sc, hit_tri);
            const F3 p = hp;
            const float cos_wi = dot(f3(-dir.x, -dir.y, -dir.z), n);
            if (!vp.only_vrl || (first_ok && second_ok)) {   // :319-350 (ESmooth diffuse)
                (void)smp.next(); (void)smp.next();
                float val[3];
                F3 ld;
                light_direct(sc, vp, p, true, val, &ld);
                if (!(val[0] == 0 && val[1] == 0 && val[2] == 0)) {
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
            const F3 wol = cosine_hemisphere(bx, by);
            F3 fs, ft;
            frame_of(n, &fs, &ft);
            const F3 wo = add(add(mul(fs, wol.x), mul(ft, wol.y)), mul(n, wol.z));
            if (depth == 1 && vp.vol_to_surf) first_ok = true;   // :377-382 (inside the medium, smooth)
            prev_volume = false;
            prev_diffuse = true;
            for (int i = 0; i < 3; i++) thr[i] *= alb[i];
            o = p; dir = wo;
            its_t = first_hit(sc, o, dir, 1e-4f, &n, &hp, &hit_tri);
            if (!indirect) break;
        }
        if (depth++ >= vp.rr_depth) {   // :437-446
            float mx = thr[0] > thr[1] ? thr[0] : thr[1];
            mx = mx > thr[2] ? mx : thr[2];
            float q = mx * eta * eta;
            if (q > 0.95f) q = 0.95f;
            if (smp.next() >= q) break;
            const float rq = 1.0f / q;
            for (int i = 0; i < 3; i++) thr[i] *= rq;
        }
    }
    if (vp.only_vrl && !(first_ok && second_ok)) Li[0] = Li[1] = Li[2] = 0.0f;   // :453-455
}

__global__ void __launch_bounds__(256) k_volpath(TCam c, TScene sc, VParams vp, uint32_t seed, uint32_t pass,
                                                 uint32_t spp, const uint32_t* __restrict__ pix, uint32_t n,
                                                 float* __restrict__ out)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t id = pix ? pix[i] : i;
    const float px = (float)(id % c.width) + 0.5f, py = (float)(id / c.width) + 0.5f;
    const float sx = px * c.inv_w, sy = py * c.inv_h;
    const float xc = (1.0f - 2.0f * sx) * c.tanh_;
    const float yc = ((1.0f - 2.0f * sy) / c.aspect) * c.tanh_;
    F3 dc = f3(xc, yc, 1.0f);
    dc = mul(dc, 1.0f / len(dc));
    const float mint = 1e-2f * (1.0f / dc.z);
    const F3 O = f3(c.o[0], c.o[1], c.o[2]);
    const F3 D = f3(c.left[0] * dc.x + c.nup[0] * dc.y + c.fwd[0] * dc.z,
                    c.left[1] * dc.x + c.nup[1] * dc.y + c.fwd[1] * dc.z,
                    c.left[2] * dc.x + c.nup[2] * dc.y + c.fwd[2] * dc.z);
    float acc[3] = {0.0f, 0.0f, 0.0f};
    for (uint32_t s = 0; s < spp; s++) {
        VStream smp{seed, pass, id, s, 0u, 0xFFFFFFFFu, {0, 0, 0, 0}};
        float li[3];
        volpath_li(sc, vp, smp, O, D, mint, li);
        for (int k = 0; k < 3; k++) acc[k] += li[k];
    }
    const float r = 1.0f / (float)spp;
    for (int k = 0; k < 3; k++) out[3 * (size_t)i + k] = acc[k] * r;
}

TScene make_tscene(const alvrl::host::SmokeBox& box)
{
    TScene sc;
    sc.light_pos[0] = box.light_pos.x; sc.light_pos[1] = box.light_pos.y; sc.light_pos[2] = box.light_pos.z;
    for (int i = 0; i < 3; i++) {
        sc.power[i] = box.light_intensity[i] * (float)(4 * kPi);
        sc.box_min[i] = box.box_min[i]; sc.box_max[i] = box.box_max[i];
        sc.albedo[i] = box.albedo[i];
        sc.sigma_s[i] = box.medium.sigma_s[i];
        sc.sigma_t[i] = box.medium.sigma_t[i];
        sc.occ_albedo[i] = box.occ_albedo[i];
    }
    sc.occ_alb = nullptr;   // set by the caller that uploads box.occ_alb (upload_albedos)
    sc.occ_mat = nullptr;   // set by the caller that uploads box.occ_mat (upload_materials)
    for (int i = 0; i < 3; i++) sc.occ_spec[i] = box.occ_spec[i];
    sc.occ_eta = box.occ_eta;
    sc.w = box.medium.sampling_weight;
    sc.strategy = box.medium.strategy;
    sc.density = box.medium.density;
    for (int i = 0; i < 3; i++) {
        sc.mx_sigma[i] = box.medium.mx_sigma[i]; sc.mx_start[i] = box.medium.mx_start[i];
        sc.mx_lower[i] = box.medium.mx_lower[i];
    }
    for (int i = 0; i < 4; i++) sc.mx_cdf[i] = box.medium.mx_cdf[i];
    sc.mx_norm = box.medium.mx_norm;
    sc.mx_inv_norm = box.medium.mx_inv_norm;
    sc.sigma_s_zero = (sc.sigma_s[0] == 0 && sc.sigma_s[1] == 0 && sc.sigma_s[2] == 0) ? 1 : 0;
    sc.bv = alvrl::bvh::View{nullptr, nullptr, nullptr, 0u};
    sc.emit = nullptr;
    sc.emit_cdf = nullptr;
    sc.nemit = (uint32_t)(box.emit.size() / 9);
    for (int i = 0; i < 3; i++) sc.emit_radiance[i] = box.emit_radiance[i];
    sc.emit_area = box.emit_area;
    return sc;
}

TCam make_tcam(const alvrl::host::SmokeBox& box, int scat)
{
    using namespace alvrl::host;
    TCam c;
    const V3 fwd = normalize(box.cam_target - box.cam_origin);
    const V3 left = normalize(cross(box.cam_up, fwd));
    const V3 nup = cross(fwd, left);
    const float vv[4][3] = {{box.cam_origin.x, box.cam_origin.y, box.cam_origin.z}, {fwd.x, fwd.y, fwd.z},
                            {left.x, left.y, left.z}, {nup.x, nup.y, nup.z}};
    for (int k = 0; k < 3; k++) { c.o[k] = vv[0][k]; c.fwd[k] = vv[1][k]; c.left[k] = vv[2][k]; c.nup[k] = vv[3][k]; }
    c.aspect = (float)box.width / (float)box.height;
    c.tanh_ = std::tan(0.5f * box.fov_x_deg * (float)(kPi / 180.0));
    c.inv_w = 1.0f / (float)box.width;
    c.inv_h = 1.0f / (float)box.height;
    c.width = (uint32_t)box.width;
    c.scat = scat;
    return c;
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
    const TCam c = make_tcam(box, 1);
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
    const TCam c = make_tcam(box, medium_scatters && !sc.sigma_s_zero ? 1 : 0);
    hipStream_t st = (hipStream_t)stream;
    const uint32_t total = n * spp;
    hipLaunchKernelGGL(k_eye_records, dim3((total + 255) / 256), dim3(256), 0, st, c, sc, d_pixel_ids, n, spp, seed,
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
    using alvrl::host::kRecWords;
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
    const bool scat = medium_scatters && !sc.sigma_s_zero;
    const TCam c = make_tcam(box, scat ? 1 : 0);
    CArgs a;
    a.seed = seed; a.pass = pass; a.sample = sample; a.spp = spp;
    a.flags = 1u | (scat ? 4u : 0u);
    a.cap = stack_cap ? std::min(stack_cap, kChainStackMax) : kChainStackDefault;
    a.spec_rr_depth = spec_rr_depth;
    a.init_thr = init_throughput;
    hipStream_t st = (hipStream_t)stream;
    // the stack workspace serves one launch of at most 2^18 lanes at a time
    const uint32_t lanes = std::min<uint32_t>(n, 1u << 18);
    DMem<float> d_stack;
    DMem<uint32_t> d_cnt, d_ovf, d_novf;
    if (d_stack.alloc((size_t)lanes * a.cap * kChainNodeWords) != hipSuccess || d_cnt.alloc(n) != hipSuccess ||
        d_ovf.alloc(n) != hipSuccess || d_novf.alloc(1) != hipSuccess)
        return terr(ALVRL_ERR_NOMEM, "alvrl_scene_chains_gpu: device memory");
    if (hipMemsetAsync(d_novf.p, 0, 4, st) != hipSuccess) return terr(ALVRL_ERR_HIP, "alvrl_scene_chains_gpu: clear");
    for (uint32_t i0 = 0; i0 < n; i0 += lanes) {
        hipLaunchKernelGGL(k_chain_count, dim3((lanes + 255) / 256), dim3(256), 0, st, c, sc, a, d_pixel_ids, i0, lanes, n,
                           d_stack.p, d_cnt.p, d_ovf.p, d_novf.p);
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
                           d_stack.p, d_cnt.p, d_base.p, d_pos.p, reinterpret_cast<float*>(d_recs), d_src);
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
    if (sc.sigma_s_zero) { *particles = 1000001; return ALVRL_OK; }   // the host loop's bound
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
