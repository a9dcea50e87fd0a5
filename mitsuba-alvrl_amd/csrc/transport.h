// transport.h -- the one source of the transport code that the host tracer
// (csrc/host/scene.cpp, g++) and the device tracer (csrc/tracer.hip, hipcc)
// both run: the Philox counter streams, the homogeneous medium's distance
// sampling, the warps, the hit record, the emitter and sensor samples, the
// gather record, vrlTracer's particle walk and one LiInternal call of the eye
// path, over the 3-vector and the triangle test of vec3.h.  Like detmath.h it
// is compiled by both compilers, so the two sides agree bit for bit by
// construction rather than by two copies kept in step.  Include it ONLY from
// translation units built with -ffp-contract=off and IEEE division / square
// root (it includes detmath.h); the gather's BVH queries take vec3.h alone.
// sin and cos are taken in double and rounded once (each side's own library),
// exp and log come from detmath.h.  No HIP header on the g++ side, no STL.
//
// What differs between the two sides is a template parameter:
//   Scene   a SceneView plus closest_occluder(): the host loops over the
//           triangles in index order, the device walks the BVH
//   Store   where an accepted VRL goes (vectors, a count, SoA planes)
//   Stack   the pending siblings of the eye-path walk (growable, or capped)
//   Out     where record k of an eye path goes
#ifndef ALVRL_TRANSPORT_H
#define ALVRL_TRANSPORT_H

#include "detmath.h"
#include "vec3.h"

namespace alvrl {
namespace transport {

constexpr double kPi = 3.14159265358979323846;

// the domains of the counter streams (seed, pass, dom, a, b, c)
constexpr uint32_t kDomTracer = 3u;    // particle p: a, b = its index
constexpr uint32_t kDomReps = 4u;      // the preprocessor's representatives: a = slice
constexpr uint32_t kDomVolpath = 6u;   // the volpath reference: a = pixel, b = sample
constexpr uint32_t kDomEye = 7u;       // Russian roulette of the eye paths' specular chains
constexpr uint32_t kDomPixel = 8u;     // sensor sample offsets of multi-sample renders

// words of a gather record (alvrl_gather_rec): o, d, p, n, albedo, flags,
// path weight (3), eye-path depth
constexpr int kRecWords = 20;

TP_FN float safe_sqrt(float v) { return sqrtf(v > 0.0f ? v : 0.0f); }
// math::fastexp / fastlog (math.h:185-199) with the deterministic definitions
// the oracle shares (detmath.h, DESIGN.md section 8 deviation 3)
TP_FN float fastexp(float v) { return dm_expf(v); }
TP_FN float fastlog(float v) { return dm_logf(v); }
TP_FN float max3(const float v[3])
{
    const float mx = v[0] > v[1] ? v[0] : v[1];
    return mx > v[2] ? mx : v[2];
}
TP_FN bool is_zero(const float v[3]) { return v[0] == 0 && v[1] == 0 && v[2] == 0; }

// ------------------------------------------------------------------ stream --
// Random123 Philox4x32-10
TP_FN void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t out[4])
{
    for (int r = 0; r < 10; r++) {
        if (r > 0) { k0 += 0x9E3779B9u; k1 += 0xBB67AE85u; }
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c0 = n0; c1 = (uint32_t)p1; c2 = n2; c3 = (uint32_t)p0;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

TP_FN float next_float(uint32_t bits)   // Random::nextFloat, random.cpp:630-639
{
    const uint32_t u = (bits >> 9) | 0x3f800000u;
    float f;
    __builtin_memcpy(&f, &u, 4);
    return f - 1.0f;
}

struct Stream {   // Sampler::next1D over the (dom, a, b, c) Philox stream
    uint32_t seed, pass, a, b, domc, k = 0;   // domc: the counter word (dom << 24) | c; k: draws taken
    uint32_t buf[4];
    TP_M Stream(uint32_t seed_, uint32_t pass_, uint32_t dom, uint32_t a_, uint32_t b_, uint32_t c = 0u)
        : seed(seed_), pass(pass_), a(a_), b(b_), domc((dom << 24) | (c & 0xFFFFFFu)), buf{0, 0, 0, 0} {}
    TP_M float next()
    {
        if ((k & 3u) == 0u) philox4x32_10(a, b, k >> 2, domc, seed, pass, buf);   // draws 4j .. 4j + 3 are block j
        return next_float(buf[k++ & 3]);
    }
};

// draws 0 and 1 of Stream(seed, pass, dom, a, b)
TP_FN void stream_draws2(uint32_t seed, uint32_t pass, uint32_t dom, uint32_t a, uint32_t b, float u[2])
{
    uint32_t buf[4];
    philox4x32_10(a, b, 0u, dom << 24, seed, pass, buf);
    u[0] = next_float(buf[0]);
    u[1] = next_float(buf[1]);
}

// ------------------------------------------------------------------ medium --
// std::max(0, lower_bound(a, a + n, x) - a - 1)
TP_FN int interval_of(const float* a, int n, float x)
{
    int k = 0;
    while (k < n && a[k] < x) k++;
    return k > 0 ? k - 1 : 0;
}

// HomogeneousMedium (src/medium/homogeneous.cpp); resolve() and problem() are
// the host's (host/scene.cpp), the sampling members run on both sides
struct MediumParams {
    float sigma_s[3] = {0.8f, 0.6f, 0.4f};
    float sigma_a[3] = {0.05f, 0.05f, 0.05f};
    float sigma_t[3] = {0.85f, 0.65f, 0.45f};
    float sampling_weight = -1.0f;   // resolved by resolve()
    int phase_type = 0;              // 0 isotropic, 1 HG
    float phase_g = 0.0f;
    int strategy = 0;                // ALVRL_STRATEGY_* (homogeneous.cpp:150-227)
    int channel = 0;                 // 'single': 1 + channel (0: the smallest sigma_t)
    float density = 0.0f;            // 'manual': samplingDensity; after resolve() m_samplingDensity
    // MaxExpDist (maxexp.h:28-94) after resolve(): sigma_t sorted decreasingly,
    // the normalised CDF at the interval starts, the starts, the lower terms
    float mx_sigma[3] = {0, 0, 0}, mx_cdf[4] = {0, 0, 0, 0}, mx_start[3] = {0, 0, 0}, mx_lower[3] = {0, 0, 0};
    float mx_norm = 0.0f, mx_inv_norm = 0.0f;
    const char* problem() const;     // what resolve() cannot accept, or nullptr
    void resolve();                  // sigma_t, the auto sampling weight (:168-184), the strategy's terms

    TP_M bool scatters() const { return !is_zero(sigma_s); }

    TP_M float maxexp_sample(float u, float* pdf) const   // maxexp.h:59-73
    {
        // the index clamped to the last interval (u = 1 above a rounded m_cdf[n])
        int i = interval_of(mx_cdf, 4, u);
        if (i > 2) i = 2;
        const float t = -fastlog(fastexp(-mx_start[i] * mx_sigma[i]) - mx_norm * (u - mx_cdf[i])) / mx_sigma[i];
        *pdf = mx_sigma[i] * fastexp(-mx_sigma[i] * t) * mx_inv_norm;
        return t;
    }

    TP_M float maxexp_cdf(float t) const   // maxexp.h:83-94
    {
        const int i = interval_of(mx_start, 3, t);
        const float upper = -fastexp(-mx_sigma[i] * t);
        return mx_cdf[i] + (upper - mx_lower[i]) * mx_inv_norm;
    }

    // sampleDistance's pdfs at the distance used (:317-346), the sampling weight
    // applied; pdf_max: MaxExpDist::sample's pdf ('maximum')
    TP_M void pdfs(float sampled, float pdf_max, float* ps, float* pf) const
    {
        const float w = sampling_weight;
        float s = 0.0f, f = 0.0f;
        if (strategy == 3) {
            f = 1 - maxexp_cdf(sampled);
            s = pdf_max;
        } else if (strategy == 0) {
            for (int i = 0; i < 3; i++) {
                const float tmp = fastexp(-sigma_t[i] * sampled);
                f += tmp;
                s += sigma_t[i] * tmp;
            }
            f /= 3; s /= 3;
        } else {
            f = fastexp(-density * sampled);
            s = density * f;
        }
        *ps = s * w;
        *pf = w * f + (1 - w);
    }

    // sampleDistance's draws (:277-296): the distance (INFINITY: no medium
    // interaction) and, for 'maximum', the pdf of the sample
    template <class S>
    TP_M float sample_distance(S& smp, float* pdf_max) const
    {
        float rnd = smp.next();
        const float w = sampling_weight;
        if (!(rnd < w)) return INFINITY;
        rnd /= w;
        if (strategy == 3) return maxexp_sample(1 - rnd, pdf_max);
        float dens = density;
        if (strategy == 0) {   // a random channel each time
            int ch = (int)(smp.next() * 3);
            if (ch > 2) ch = 2;
            dens = sigma_t[ch];
        }
        return -fastlog(1 - rnd) / dens;
    }

    // Medium::eval over a segment of length t, with the 1e-20 cut-off (:352)
    TP_M void transmittance(float t, float tr[3]) const
    {
        for (int i = 0; i < 3; i++) tr[i] = fastexp(sigma_t[i] * (-t));
        if (max3(tr) < 1e-20f) tr[0] = tr[1] = tr[2] = 0;
    }

    // sampleDistance over a ray whose surface hit is at its_t (:275-352): the
    // medium interaction's point (true) or the surface (false), the pdfs and
    // the transmittance at the distance used
    template <class S>
    TP_M bool sample_segment(S& smp, V3 o, V3 dir, float its_t, V3* mp, float* ps, float* pf, float mtr[3]) const
    {
        float pdf_max = 0.0f;
        float sampled = sample_distance(smp, &pdf_max);
        const float distSurf = its_t - 0.0f;
        bool success = true;
        *mp = o;
        if (sampled < distSurf) {
            *mp = o + dir * (sampled + 0.0f);
            if (mp->x == o.x && mp->y == o.y && mp->z == o.z) success = false;
        } else {
            sampled = distSurf;
            success = false;
        }
        pdfs(sampled, pdf_max, ps, pf);
        transmittance(sampled, mtr);
        return success;
    }
};

// ------------------------------------------------------------------- warps --
TP_FN V3 uniform_sphere(float sx, float sy)   // warp.cpp:25-31
{
    const float z = 1.0f - 2.0f * sy;
    const float r = safe_sqrt(1.0f - z * z);
    const float theta = (float)(2.0f * kPi * sx);
    // sin/cos in double, rounded once (the oracle does the same)
    return v3(r * (float)cos((double)theta), r * (float)sin((double)theta), z);
}

TP_FN V3 cosine_hemisphere(float sx, float sy)   // warp.cpp:43-52, 81-102
{
    const float r1 = 2.0f * sx - 1.0f, r2 = 2.0f * sy - 1.0f;
    float phi, r;
    if (r1 == 0 && r2 == 0) { r = phi = 0; }
    else if (r1 * r1 > r2 * r2) { r = r1; phi = (float)((kPi / 4.0f) * (r2 / r1)); }
    else { r = r2; phi = (float)((kPi / 2.0f) - (r1 / r2) * (kPi / 4.0f)); }
    const float px = r * (float)cos((double)phi), py = r * (float)sin((double)phi);
    float z = safe_sqrt(1.0f - px * px - py * py);
    if (z == 0) z = 1e-10f;
    return v3(px, py, z);
}

struct Frame {
    V3 s, t, n;
    TP_M V3 to_world(V3 l) const { return (s * l.x + t * l.y) + n * l.z; }
    // reflect(wi) / -wi / refract(wi, cosThetaT) of the local wi = -(-mwi): the
    // x and y components scaled, z given
    TP_M V3 local(V3 mwi, float scale, float z) const { return v3(scale * dot(mwi, s), scale * dot(mwi, t), z); }
};

TP_FN Frame frame_of(V3 a)   // Frame(n) by coordinateSystem, util.cpp:592-601
{
    Frame f;
    f.n = a;
    if (fabsf(a.x) > fabsf(a.y)) {
        const float invLen = 1.0f / sqrtf(a.x * a.x + a.z * a.z);
        f.t = v3(a.z * invLen, 0.0f, -a.x * invLen);
    } else {
        const float invLen = 1.0f / sqrtf(a.y * a.y + a.z * a.z);
        f.t = v3(0.0f, a.z * invLen, -a.y * invLen);
    }
    f.s = cross(f.t, a);
    return f;
}

// fresnelDielectricExt (src/libcore/util.cpp:651-681): unpolarized Fresnel
// reflectance and the signed cosine of the transmitted direction.
TP_FN float fresnel_dielectric_ext(float cos_theta_i, float* cos_theta_t, float eta)
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

// ------------------------------------------------------------------- scene --
// What the walks read of a SmokeBox (host/scene.hpp); the pointers are host or
// device memory.  A Scene adds
//   const float* closest_occluder(o, d, mint, &best, &id, &u, &v) const
// the closest triangle hit with t in [mint, *best) -- the walls win ties, then
// the lowest index -- updating best, id (the triangle's index) and the
// barycentrics, and returning the triangle's 9 floats.
struct SceneView {
    float light_pos[3], power[3];   // the point light: intensity * 4 pi
    float box_min[3], box_max[3], albedo[3];
    MediumParams medium;
    float occ_albedo[3];
    const float* occ_alb;           // per-triangle reflectance (3 floats each), or nullptr: occ_albedo for all
    const uint32_t* occ_mat;        // per-triangle ALVRL_MAT_*, or nullptr: every triangle diffuse
    float occ_spec[3], occ_eta;     // the mirrors' reflectance, the dielectrics' intIOR / extIOR
    // area emitter (nemit == 0: the point light): triangles, the normalized
    // area CDF (nemit + 1 entries), radiance and surface area
    const float* emit;
    const float* emit_cdf;
    uint32_t nemit;
    float emit_radiance[3], emit_area;

    // the diffuse reflectance of a hit: the occluder's own or the shared one, or the walls' (tri < 0)
    TP_M const float* albedo_of(int tri) const
    {
        return tri < 0 ? albedo : occ_alb ? occ_alb + 3 * (size_t)tri : occ_albedo;
    }
    // the BSDF of a hit: 0 diffuse (the walls too), 1 mirror, 2 null, 3 dielectric
    TP_M uint32_t mat(int tri) const { return (tri < 0 || !occ_mat) ? 0u : occ_mat[(size_t)tri]; }
};

// First hit of a ray starting inside the box: t and inward normal.
TP_FN float box_hit(const SceneView& sc, V3 o, V3 d, V3* n)
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
    *n = v3(nn[0], nn[1], nn[2]);
    return best;
}

// Scene::rayIntersect over the walls and the occluders, t >= mint.  *tri = -1
// for a wall; *p = its.p (ray(t) for a wall, barycentric for a triangle).
template <class Scene>
TP_FN float first_hit(const Scene& sc, V3 o, V3 d, float mint, V3* n, V3* p, int* tri)
{
    float best = box_hit(sc, o, d, n);
    int id = -1;
    float bu = 0.0f, bv = 0.0f;
    const float* q = sc.closest_occluder(o, d, mint, &best, &id, &bu, &bv);
    *tri = id;
    if (id < 0) {
        *p = o + d * best;
        return best;
    }
    // fillIntersectionRecord (skdtree.h:350-396): barycentric position, face normal
    const V3 p0 = v3(q[0], q[1], q[2]), p1 = v3(q[3], q[4], q[5]), p2 = v3(q[6], q[7], q[8]);
    const float b0 = 1 - bu - bv;
    *p = (p0 * b0 + p1 * bu) + p2 * bv;
    V3 fn = cross(p1 - p0, p2 - p0);
    const float len = length(fn);
    if (!(fn.x == 0 && fn.y == 0 && fn.z == 0)) fn = fn * (1.0f / len);
    *n = fn;
    return best;
}

// Scene::sampleEmitterPosition + Emitter::sampleDirection of the area emitter
// for the tracer's draws (sx, sy) and (dx, dy): origin, direction and power
// (vrlTracer.h:109-120)
TP_FN V3 area_emission(const SceneView& sc, float sx, float sy, float dx, float dy, V3* dir, float power[3])
{
    // Scene::sampleEmitterPosition: one emitter, so m_emitterPDF.sampleReuse
    // leaves sample.x as it is and the pdf is 1 (pmf.h:124-169)
    // TriMesh::samplePosition: the triangle by m_areaDistr.sampleReuse(sample.y)
    const uint32_t n = sc.nemit;
    uint32_t lb = 0;
    while (lb <= n && sc.emit_cdf[lb] < sy) lb++;   // std::lower_bound
    uint32_t idx = lb > 0 ? lb - 1 : 0;
    if (idx > n - 1) idx = n - 1;
    // a zero-area triangle is skipped (the reference's loop would read past the table
    // if the last one had zero area)
    while (idx + 1 < n && sc.emit_cdf[idx + 1] - sc.emit_cdf[idx] == 0) ++idx;
    const float y = (sy - sc.emit_cdf[idx]) / (sc.emit_cdf[idx + 1] - sc.emit_cdf[idx]);
    // Triangle::sample with warp::squareToUniformTriangle (warp.cpp:76-79)
    const float a = safe_sqrt(1.0f - sx);
    const float bx = 1 - a, by = a * y;
    const float* t = sc.emit + 9 * (size_t)idx;
    const V3 p0 = v3(t[0], t[1], t[2]);
    const V3 sideA = v3(t[3], t[4], t[5]) - p0, sideB = v3(t[6], t[7], t[8]) - p0;
    const V3 nn = normalize(cross(sideA, sideB));
    // AreaEmitter::samplePosition returns m_power = m_radiance * M_PI * area
    // (area.cpp:94-98, 198); sampleDirection: a cosine-weighted direction in
    // Frame(pRec.n), weight 1 (area.cpp:115-123)
    for (int i = 0; i < 3; i++) power[i] = (sc.emit_radiance[i] * (float)kPi) * sc.emit_area;
    *dir = frame_of(nn).to_world(cosine_hemisphere(dx, dy));
    return (p0 + sideA * bx) + sideB * by;
}

// ------------------------------------------------------------------ sensor --
// The perspective camera's per-scene terms (perspective.cpp:126-155), formed
// on the host (SmokeBox::camera).
struct Camera {
    V3 o, fwd, left, nup;
    float tanh_, aspect, inv_w, inv_h;
    uint32_t width;
};

// Sensor::sampleRay through pixel sample (px, py); *mint = nearClip / d.z in
// camera space (perspective.cpp:247-263, nearClip 1e-2).
TP_FN void camera_ray(const Camera& c, float px, float py, V3* o, V3* d, float* mint)
{
    const float sx = px * c.inv_w, sy = py * c.inv_h;
    const float xc = (1.0f - 2.0f * sx) * c.tanh_;
    const float yc = ((1.0f - 2.0f * sy) / c.aspect) * c.tanh_;
    const V3 dc = normalize(v3(xc, yc, 1.0f));
    *mint = 1e-2f * (1.0f / dc.z);
    *o = c.o;
    *d = v3(c.left.x * dc.x + c.nup.x * dc.y + c.fwd.x * dc.z,
            c.left.y * dc.x + c.nup.y * dc.y + c.fwd.y * dc.z,
            c.left.z * dc.x + c.nup.z * dc.y + c.fwd.z * dc.z);
}

// The sensor ray of pixel id (row-major), sample j of spp (renderBlock,
// integrator.cpp:240-247): through the pixel centre for one sample per pixel,
// else through (x, y) + rRec.nextSample2D(), here draws 0 and 1 of the stream
// (seed, pass, dom 8, pixel, j).
TP_FN void sensor_ray(const Camera& c, uint32_t id, uint32_t j, uint32_t spp, uint32_t seed, uint32_t pass, V3* o,
                      V3* d, float* mint)
{
    float u[2] = {0.5f, 0.5f};
    if (spp > 1) stream_draws2(seed, pass, kDomPixel, id, j, u);
    camera_ray(c, (float)(id % c.width) + u[0], (float)(id / c.width) + u[1], o, d, mint);
}

// ------------------------------------------------------------------ record --
// One gather record (alvrl_gather_rec); diffuse false: the reflectance words
// are zero (a delta BSDF, or no reflectance wanted).
TP_FN void write_record(float* r, V3 o, V3 d, V3 p, V3 n, const float albedo[3], bool diffuse, uint32_t flags,
                        const float w[3], uint32_t depth_word)
{
    r[0] = o.x; r[1] = o.y; r[2] = o.z;
    r[3] = d.x; r[4] = d.y; r[5] = d.z;
    r[6] = p.x; r[7] = p.y; r[8] = p.z;
    r[9] = n.x; r[10] = n.y; r[11] = n.z;
    for (int i = 0; i < 3; i++) r[12 + i] = diffuse ? albedo[i] : 0.0f;
    __builtin_memcpy(&r[15], &flags, 4);
    for (int i = 0; i < 3; i++) r[16 + i] = w[i];
    __builtin_memcpy(&r[19], &depth_word, 4);
}

// The record of the sensor ray of pixel id, sample j of spp: path weight 1,
// depth word j << 16.  flags: HIT and ESmooth (diffuse) or EDelta when the ray
// hits, MEDIUM when the medium scatters.
template <class Scene>
TP_FN void primary_record(const Scene& sc, const Camera& c, bool medium_scatters, uint32_t id, uint32_t j, uint32_t spp,
                          uint32_t seed, uint32_t pass, float* r)
{
    V3 O, D, n, p;
    float mint;
    sensor_ray(c, id, j, spp, seed, pass, &O, &D, &mint);
    int tri;
    const float t = first_hit(sc, O, D, mint, &n, &p, &tri);
    const uint32_t m = sc.mat(tri);
    uint32_t flags = 0;
    if (isfinite(t)) flags |= 1u | (m == 0u ? 2u : 8u);
    if (medium_scatters) flags |= 4u;
    const float one[3] = {1.0f, 1.0f, 1.0f};
    write_record(r, O, D, p, n, sc.albedo_of(tri), m == 0u, flags, one, j << 16);
}

// ----------------------------------------------------------- particle walk --
// vrlVector::put + the tracer's current VRL (vrlTracer.h:56-89, VRL.h:148-158).
// Store::add(start, end, power) takes a VRL that passes the put-filter.
template <class Store>
struct Sink {
    V3 start;
    float power[3];
    bool sigma_s_zero;
    Store store;
    TP_M void put(V3 end)
    {
        if (sigma_s_zero) return;
        if (is_zero(power)) return;
        if (length(start - end) == 0) return;
        store.add(start, end, power);
    }
    TP_M void end_current(V3 p)
    {
        if (length(start - p) == 0) return;
        put(p);
    }
    TP_M void begin(V3 p, const float thr[3], const float emitted[3])
    {
        start = p;
        for (int i = 0; i < 3; i++) power[i] = thr[i] * emitted[i];
    }
};

// vrlTracer::randomWalk's particle (vrlTracer.h:91-230), with the counter
// stream smp instead of one sequential sampler.
template <class Scene, class S, class Store>
TP_FN void trace_particle(const Scene& sc, S& smp, bool short_vrls, int max_depth, int rr_depth, Sink<Store>& k)
{
    const MediumParams& m = sc.medium;
    const float sx = smp.next(), sy = smp.next();   // sampleEmitterPosition (scene.cpp:958-974)
    const float dx = smp.next(), dy = smp.next();   // sampleDirection (point.cpp:99-106, area.cpp:115-123)
    float power[3];
    V3 dir, o;
    if (sc.nemit) {
        o = area_emission(sc, sx, sy, dx, dy, &dir, power);
    } else {
        dir = uniform_sphere(dx, dy);
        o = v3(sc.light_pos[0], sc.light_pos[1], sc.light_pos[2]);
        for (int i = 0; i < 3; i++) power[i] = sc.power[i];
    }
    if (is_zero(power)) return;
    k.start = o;
    for (int i = 0; i < 3; i++) k.power[i] = power[i];
    int depth = 1;
    float thr[3] = {1.0f, 1.0f, 1.0f};
    float eta = 1.0f;
    float mint = 1e-4f;   // Ray() default mint (Epsilon), then 0 after a medium and Epsilon after a surface
    // bounded by max_depth when set, else by the roulette from rr_depth on
    // (survival <= 0.95 per iteration) and the throughput reaching 0
    while (!is_zero(thr) && (depth <= max_depth || max_depth < 0)) {
        V3 n, hp, mp;
        int tri;
        const float its_t = first_hit(sc, o, dir, mint, &n, &hp, &tri);
        float pf, ps, mtr[3];
        if (m.sample_segment(smp, o, dir, its_t, &mp, &ps, &pf, mtr)) {   // vrlTracer.h:143-172
            const float rps = 1.0f / ps;
            for (int i = 0; i < 3; i++) thr[i] *= mtr[i] * m.sigma_s[i] * rps;
            const float px_ = smp.next(), py_ = smp.next();
            const V3 wo = uniform_sphere(px_, py_);
            k.end_current(short_vrls ? mp : hp);
            k.begin(mp, thr, power);
            o = mp; dir = wo; mint = 0.0f;
        } else if (isfinite(its_t)) {   // vrlTracer.h:173-213
            const float rpf = 1.0f / pf;
            for (int i = 0; i < 3; i++) thr[i] *= mtr[i] * rpf;
            const V3 p = hp;
            const float* alb = sc.albedo_of(tri);
            const Frame fr = frame_of(n);
            const V3 mwi = -dir;
            const float cos_wi = dot(mwi, n);
            const float bx = smp.next(), by = smp.next();   // bsdf->sample(bRec, next2D())
            float bw[3] = {0, 0, 0};
            V3 wol = v3(0, 0, 0);
            const uint32_t mt = sc.mat(tri);
            if (mt == 0u) {          // SmoothDiffuse::sample (diffuse.cpp:120-133)
                if (!(cos_wi <= 0)) {
                    wol = cosine_hemisphere(bx, by);
                    for (int i = 0; i < 3; i++) bw[i] = alb[i];
                }
            } else if (mt == 1u) {   // SmoothConductor::sample (conductor.cpp:254-268), material none
                if (!(cos_wi <= 0)) {
                    wol = fr.local(mwi, -1.0f, cos_wi);   // reflect(wi)
                    for (int i = 0; i < 3; i++) bw[i] = sc.occ_spec[i];
                }
            } else if (mt == 3u) {   // SmoothDielectric::sample, both components, EImportance (dielectric.cpp:335-364)
                float cos_t;
                const float F = fresnel_dielectric_ext(cos_wi, &cos_t, sc.occ_eta);
                if (bx <= F) {
                    wol = fr.local(mwi, -1.0f, cos_wi);
                } else {
                    const float inv_eta = 1 / sc.occ_eta;
                    wol = fr.local(mwi, -(cos_t < 0 ? inv_eta : sc.occ_eta), cos_t);   // refract(wi, cosThetaT)
                    eta *= cos_t < 0 ? sc.occ_eta : inv_eta;                            // bRec.eta
                }
                bw[0] = bw[1] = bw[2] = 1.0f;                                          // importance: factor 1
            } else {                 // Null::sample (null.cpp:53-63): wo = -wi
                wol = fr.local(mwi, -1.0f, -cos_wi);
                bw[0] = bw[1] = bw[2] = 1.0f;
            }
            if (is_zero(bw)) { k.end_current(p); break; }
            const V3 wo = fr.to_world(wol);
            const float wiDotGeoN = dot(n, mwi), woDotGeoN = dot(n, wo);
            if (wiDotGeoN * cos_wi <= 0 || woDotGeoN * wol.z <= 0) { k.end_current(p); break; }
            for (int i = 0; i < 3; i++) thr[i] *= bw[i];
            k.end_current(p);
            k.begin(p, thr, power);
            o = p; dir = wo; mint = 1e-4f;
        } else {
            break;
        }
        if (depth++ >= rr_depth) {
            float q = max3(thr) * eta * eta;
            if (q > 0.95f) q = 0.95f;
            if (smp.next() >= q) break;
            const float rq = 1.0f / q;
            for (int i = 0; i < 3; i++) thr[i] *= rq;
        }
    }
}

// --------------------------------------------------------------- eye paths --
// LiInternal's recursion through delta BSDFs (vrlIntegrator.cpp:386-524) as
// gather records, one per segment, each with the weight the recursion passes
// down (:503-510), in an explicit pre-order traversal.  A node is one
// LiInternal call: the record of the ray's hit, then each delta component's
// continuation (bRec.component = i, :467-511): a dielectric branches into
// reflection and transmission, so the records form a tree, emitted depth
// first (component 0's subtree before component 1's).  Record k (pre-order
// index) has depth word k | (j << 16) for sensor sample j.  The roulette
// stream of a node is keyed by that word (seed, pass, dom 7, pixel, k | j <<
// 16) and only that node draws from it, in component order, so both children
// are decided when the node is visited: the walk goes on with the first
// surviving child and, at a dielectric whose reflection and refraction both
// survive, parks the refracted one on the Stack until the reflected subtree
// is finished.
constexpr uint32_t kChainMaxRecs = 256u;           // records per eye path
constexpr uint32_t kChainOverflow = 0xFFFFFFFFu;   // chain_walk: the Stack refused a push

struct ChainArgs {
    uint32_t seed, pass, sample, spp, flags;   // flags: HIT | MEDIUM of every record
    int spec_rr_depth;
    float init_thr;
};

struct ChainNode {
    V3 o, d;
    float w[3], thr[3];   // the path weight passed down, throughputWithEtaSq
    int depth;            // rRec.depth (1 for the sensor ray)
};

// One LiInternal call after its hit (t, n, p) on the BSDF m, record word kw
// (:447-511): the segment's transmittance, then each delta component (at most
// 2) sampled with bsdf->sample(bRec, Point2(0.5f)), its Russian roulette (from
// initialSpecularThroughput, maxRR 0.98 past specularForcedRRdepth, :475-492)
// and the node of its continuation: live[c] says whether child[c] survives.
// The loop over the components and the node's draws taken together when the
// first is needed keep the device's registers where five waves fit (DESIGN
// 5.10): two separately inlined component bodies cost ten more.
template <class Scene>
TP_FN void eye_node(const Scene& sc, const ChainArgs& a, uint32_t pixel, uint32_t kw, const ChainNode& cur, float t,
                    V3 n, V3 p, uint32_t m, ChainNode child[2], bool live[2])
{
    live[0] = live[1] = false;
    float tr[3] = {0.0f, 0.0f, 0.0f};
    // the segment's transmittance, rRec.medium->eval(Ray(ray, 0, its.t)) (:450-460); a diffuse hit has no
    // delta component (:447-448)
    if (m != 0u) sc.medium.transmittance(t, tr);
    if (is_zero(tr)) return;
    const Frame fr = frame_of(n);
    const V3 mwi = -cur.d;
    const float cos_wi = dot(mwi, n);
    float u[2] = {0.0f, 0.0f};
    bool drawn = false;
    int nd = 0;   // draws taken from this node's stream
    const int ncomp = m == 3u ? 2 : 1;
    for (int c = 0; c < ncomp; c++) {
        float bw[3];
        float beta = 1.0f;   // bRec.eta
        V3 wol;
        if (m == 1u) {          // conductor.cpp:254-268
            if (cos_wi <= 0) continue;
            wol = fr.local(mwi, -1.0f, cos_wi);
            for (int i = 0; i < 3; i++) bw[i] = sc.occ_spec[i];
        } else if (m == 2u) {   // null.cpp:53-63
            wol = fr.local(mwi, -1.0f, -cos_wi);
            bw[0] = bw[1] = bw[2] = 1.0f;
        } else {                // dielectric.cpp:365-385, one component, ERadiance
            float cos_t;
            const float F = fresnel_dielectric_ext(cos_wi, &cos_t, sc.occ_eta);
            const float inv_eta = 1 / sc.occ_eta;
            if (c == 0) {
                wol = fr.local(mwi, -1.0f, cos_wi);
                bw[0] = bw[1] = bw[2] = F;
            } else {
                wol = fr.local(mwi, -(cos_t < 0 ? inv_eta : sc.occ_eta), cos_t);
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
        const float mx = max3(thr2);
        const float rrProb = maxRR < mx ? maxRR : mx;
        if (rrProb <= 0) continue;
        if (rrProb < 1) {
            if (!drawn) { stream_draws2(a.seed, a.pass, kDomEye, pixel, kw, u); drawn = true; }
            if (u[nd++] > rrProb) continue;
        }
        ChainNode& ch = child[c];
        for (int i = 0; i < 3; i++) {
            ch.thr[i] = thr2[i] / rrProb;
            ch.w[i] = ((cur.w[i] * tr[i]) * bw[i]) / rrProb;   // weight * transmittance * bsdfWeight / rrProb (:505)
        }
        ch.o = p;
        ch.d = fr.to_world(wol);   // its.toWorld(bRec.wo)
        ch.depth = cur.depth + 1;
        live[c] = true;
    }
}

// The eye path of pixel 'pixel' from the sensor ray (O, D, mint0).  Record k
// goes to out.slot(k) (nullptr: not wanted).  Returns the number of records
// (at most kChainMaxRecs), or kChainOverflow when st.push() refuses a sibling.
template <class Scene, class Stack, class Out>
TP_FN uint32_t chain_walk(const Scene& sc, const ChainArgs& a, uint32_t pixel, V3 O, V3 D, float mint0, Stack& st,
                          Out& out)
{
    ChainNode cur;
    cur.o = O; cur.d = D;
    for (int i = 0; i < 3; i++) { cur.w[i] = 1.0f; cur.thr[i] = a.init_thr; }   // throughputWithEtaSq (:381)
    cur.depth = 1;
    float mint = mint0;
    uint32_t k = 0;
    // One iteration per visited node.  Bound: a node either writes a record
    // (at most kChainMaxRecs of them) or ends its branch and pops a sibling
    // (at most one per record written), so <= 512 iterations.
    while (k < kChainMaxRecs) {
        bool alive = false;
        ChainNode next;
        V3 n, p;
        int tri;
        const float t = first_hit(sc, cur.o, cur.d, mint, &n, &p, &tri);
        if (isfinite(t)) {   // :414-419
            const uint32_t m = sc.mat(tri);
            const uint32_t kw = k | (a.sample << 16);
            if (float* r = out.slot(k))
                write_record(r, cur.o, cur.d, p, n, sc.albedo_of(tri), m == 0u, a.flags | (m == 0u ? 2u : 8u), cur.w,
                             kw);
            ++k;
            ChainNode child[2];
            bool live[2];
            eye_node(sc, a, pixel, kw, cur, t, n, p, m, child, live);
            if (live[0] && live[1] && !st.push(child[1])) return kChainOverflow;
            if (live[0]) { next = child[0]; alive = true; }
            else if (live[1]) { next = child[1]; alive = true; }
        }
        if (!alive && !st.pop(&next)) break;
        cur = next;
        mint = 1e-4f;   // RayDifferential(its.p, wo): mint = Epsilon
    }
    return k;
}

}  // namespace transport
}  // namespace alvrl

#endif
