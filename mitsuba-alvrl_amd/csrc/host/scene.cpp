// scene.cpp -- smoke-box harness and the VRL tracer (see scene.hpp).
// Compiled with g++ -ffp-contract=off: float semantics identical to the
// oracle's restatement, so records and VRL sets agree bit for bit with it.
// The walks themselves are transport.h's, which tracer.hip compiles too.
#include "scene.hpp"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>

namespace alvrl {

namespace transport {

void MediumParams::resolve()
{
    for (int i = 0; i < 3; i++) sigma_t[i] = sigma_s[i] + sigma_a[i];
    float w = sampling_weight;
    if (w == -1) {
        for (int i = 0; i < 3; i++) {
            const float albedo = sigma_s[i] / sigma_t[i];
            if (albedo > w && sigma_t[i] != 0) w = albedo;
        }
        if (w > 0) w = w > 0.5f ? w : 0.5f;
    }
    sampling_weight = w;
    density = strategy == 2 ? density : 0.0f;
    if (strategy == 1) {   // homogeneous.cpp:188-204
        int ch = channel - 1;
        if (ch < 0) {
            float smallest = INFINITY;
            ch = 0;
            for (int i = 0; i < 3; i++)
                if (sigma_t[i] < smallest) { smallest = sigma_t[i]; ch = i; }
        }
        density = sigma_t[ch];
    } else if (strategy == 3) {   // MaxExpDist(sigmaT), maxexp.h:30-57
        float s[3] = {sigma_t[0], sigma_t[1], sigma_t[2]};
        std::sort(s, s + 3, [](float a, float b) { return a > b; });
        float cdf[4];
        cdf[0] = 0;
        for (int i = 0; i < 3; i++) {
            const float lower = (i == 0) ? -1 : -std::pow(s[i] / s[i - 1], -s[i] / (s[i] - s[i - 1]));
            const float upper = (i == 2) ? 0 : -std::pow(s[i + 1] / s[i], -s[i] / (s[i + 1] - s[i]));
            cdf[i + 1] = cdf[i] + (upper - lower);
            mx_start[i] = (i == 0) ? 0 : fastlog(s[i] / s[i - 1]) / (s[i] - s[i - 1]);
            mx_lower[i] = lower;
            mx_sigma[i] = s[i];
        }
        mx_norm = cdf[3];
        mx_inv_norm = 1 / mx_norm;
        for (int i = 0; i < 4; i++) mx_cdf[i] = cdf[i] * mx_inv_norm;
    }
}

const char* MediumParams::problem() const
{
    if (strategy < 0 || strategy > 3) return "alvrl_medium_desc: unknown sampling strategy";
    if (strategy == 1 && (channel < 0 || channel > 3)) return "alvrl_medium_desc: 'single' channel out of range";
    if (strategy == 3) {
        float s[3];
        for (int i = 0; i < 3; i++) s[i] = sigma_s[i] + sigma_a[i];
        if (s[0] == s[1] || s[1] == s[2] || s[0] == s[2])
            return "alvrl_medium_desc: 'maximum' needs sigma_t to vary across channels (maxexp.h:37-38)";
    }
    return nullptr;
}

}  // namespace transport

namespace host {

using namespace transport;

HostScene SmokeBox::view() const
{
    HostScene sc;
    sc.light_pos[0] = light_pos.x; sc.light_pos[1] = light_pos.y; sc.light_pos[2] = light_pos.z;
    for (int i = 0; i < 3; i++) {
        sc.power[i] = light_intensity[i] * (float)(4 * kPi);
        sc.box_min[i] = box_min[i]; sc.box_max[i] = box_max[i];
        sc.albedo[i] = albedo[i];
        sc.occ_albedo[i] = occ_albedo[i];
        sc.occ_spec[i] = occ_spec[i];
        sc.emit_radiance[i] = emit_radiance[i];
    }
    sc.medium = medium;
    sc.occ_alb = occ_alb.empty() ? nullptr : occ_alb.data();
    sc.occ_mat = occ_mat.empty() ? nullptr : occ_mat.data();
    sc.occ_eta = occ_eta;
    sc.emit = emit.data();
    sc.emit_cdf = emit_cdf.data();
    sc.nemit = (uint32_t)(emit.size() / 9);
    sc.emit_area = emit_area;
    sc.occ = occ.data();
    sc.nocc = n_occ();
    return sc;
}

Camera SmokeBox::camera() const
{
    Camera c;
    c.o = cam_origin;
    c.fwd = normalize(cam_target - cam_origin);
    c.left = normalize(cross(cam_up, c.fwd));
    c.nup = cross(c.fwd, c.left);
    c.aspect = (float)width / (float)height;
    c.tanh_ = std::tan(0.5f * fov_x_deg * (float)(kPi / 180.0));
    c.inv_w = 1.0f / (float)width;
    c.inv_h = 1.0f / (float)height;
    c.width = (uint32_t)width;
    return c;
}

void SmokeBox::make_record(int x, int y, bool medium_scatters, float rec[kRecWords], uint32_t seed, uint32_t pass,
                           uint32_t sample, uint32_t spp) const
{
    primary_record(view(), camera(), medium_scatters, (uint32_t)y * (uint32_t)width + (uint32_t)x, sample, spp, seed,
                   pass, rec);
}

void SmokeBox::make_slice_record(int x, int y, float rec[kRecWords]) const
{
    const HostScene sc = view();
    V3 O, D, n, p;
    float mint;
    camera_ray(camera(), (float)x + 0.5f, (float)y + 0.5f, &O, &D, &mint);
    int tri;
    float t = first_hit(sc, O, D, mint, &n, &p, &tri);
    uint32_t flags = 0;
    V3 gp = p, gn = n;
    if (std::isfinite(t)) {
        flags = 1u;
        while (true) {   // Preprocessor.cpp:1157-1169
            gp = p; gn = n;
            if (sc.mat(tri) != 2u) break;
            t = first_hit(sc, O, D, t + 1e-4f, &n, &p, &tri);   // Ray(ray, its.t + Epsilon, ray.maxt)
            if (!std::isfinite(t)) break;
        }
    }
    const float one[3] = {1.0f, 1.0f, 1.0f};
    write_record(rec, O, D, gp, gn, one, false, flags, one, 0u);
}

float SmokeBox::scene_diagonal() const
{
    const float a = box_max[0] - box_min[0], b = box_max[1] - box_min[1], c = box_max[2] - box_min[2];
    return std::sqrt(a * a + b * b + c * c);
}

// TriMesh::prepareSamplingTable (trimesh.cpp:388-403): Triangle::surfaceArea
// (triangle.cpp: 0.5 |cross(p1 - p0, p2 - p0)|) appended to a
// DiscreteDistribution (running float sum), normalized (pmf.h:101-114)
void SmokeBox::prepare_emitter()
{
    const size_t n = emit.size() / 9;
    emit_cdf.assign(1, 0.0f);
    for (size_t i = 0; i < n; i++) {
        const float* t = &emit[9 * i];
        const V3 p0 = v3(t[0], t[1], t[2]), p1 = v3(t[3], t[4], t[5]), p2 = v3(t[6], t[7], t[8]);
        const float a = 0.5f * length(cross(p1 - p0, p2 - p0));
        emit_cdf.push_back(emit_cdf.back() + a);
    }
    emit_area = emit_cdf.back();
    if (emit_area > 0) {
        const float norm = 1.0f / emit_area;
        for (size_t i = 1; i < emit_cdf.size(); i++) emit_cdf[i] *= norm;
        emit_cdf.back() = 1.0f;
    }
}

namespace {

struct ChainStack {   // the pending siblings: as deep as the tree asks for
    std::vector<ChainNode> v;
    bool push(const ChainNode& nd) { v.push_back(nd); return true; }
    bool pop(ChainNode* nd)
    {
        if (v.empty()) return false;
        *nd = v.back();
        v.pop_back();
        return true;
    }
};

struct ChainOut {   // every record, appended in pre-order
    std::vector<float>* out;
    float* slot(uint32_t)
    {
        out->resize(out->size() + kRecWords);
        return out->data() + out->size() - kRecWords;
    }
};

struct VrlStore {   // vrlVector's planes
    std::vector<float> s[9];
    void add(V3 start, V3 end, const float power[3])
    {
        const float v[9] = {start.x, start.y, start.z, end.x, end.y, end.z, power[0], power[1], power[2]};
        for (int pl = 0; pl < 9; pl++) s[pl].push_back(v[pl]);
    }
    void move_to(VrlSet* out) const
    {
        out->n = (uint32_t)s[0].size();
        out->soa.resize(9 * (size_t)out->n);
        for (int pl = 0; pl < 9; pl++)
            std::memcpy(&out->soa[(size_t)pl * out->n], s[pl].data(), sizeof(float) * out->n);
    }
};

}  // namespace

void SmokeBox::make_chain(int x, int y, bool medium_scatters, uint32_t seed, uint32_t pass, int spec_rr_depth,
                          float init_throughput, std::vector<float>* out, uint32_t sample, uint32_t spp) const
{
    const uint32_t pixel = (uint32_t)y * (uint32_t)width + (uint32_t)x;
    V3 O, D;
    float mint;
    sensor_ray(camera(), pixel, sample, spp, seed, pass, &O, &D, &mint);   // the sensor sample (integrator.cpp:240-247)
    const ChainArgs a{seed, pass, sample, spp, 1u | (medium_scatters ? 4u : 0u), spec_rr_depth, init_throughput};
    ChainStack st;
    ChainOut o{out};
    (void)chain_walk(view(), a, pixel, O, D, mint, st, o);
}

VrlSet trace_vrls(const SmokeBox& box, uint32_t seed, uint32_t pass, uint32_t target, bool short_vrls,
                  int max_depth, int rr_depth)
{
    const HostScene sc = box.view();
    Sink<VrlStore> k;
    k.sigma_s_zero = !sc.medium.scatters();
    uint64_t p = 0;
    while (k.store.s[0].size() < target) {   // vrlTracer::randomWalk, vrlTracer.h:29-39
        Stream smp(seed, pass, kDomTracer, (uint32_t)p, (uint32_t)(p >> 32));
        p++;   // handleEmission -> nextParticle (the point light always emits)
        trace_particle(sc, smp, short_vrls, max_depth, rr_depth, k);
        if (k.sigma_s_zero && p > 1000000) break;
    }
    VrlSet out;
    k.store.move_to(&out);
    out.particle_count = p;
    return out;
}

bool read_vrl_file(const char* path, const MediumParams& m, VrlSet* out, std::string* err)
{
    std::ifstream f(path);
    if (!f) { *err = std::string("cannot open VRL file ") + path; return false; }
    Sink<VrlStore> k;
    k.sigma_s_zero = !m.scatters();
    std::string line;
    while (std::getline(f, line)) {
        std::stringstream ss(line);
        float v[9];
        int got = 0;
        while (got < 9 && (ss >> v[got])) got++;
        if (got == 0) continue;
        if (got != 9) break;   // the reference stops at the first unparsable line (VRL.h:121-126)
        for (int i = 6; i < 9; i++)
            if (!std::isfinite(v[i]) || v[i] < 0) { *err = "invalid parsed VRL power"; return false; }   // VRL.h:51-53
        k.start = v3(v[0], v[1], v[2]);
        k.power[0] = v[6]; k.power[1] = v[7]; k.power[2] = v[8];
        k.put(v3(v[3], v[4], v[5]));
    }
    k.store.move_to(out);
    out->particle_count = out->n;   // m_numParticles = size() (VRL.h:127)
    return true;
}

bool write_vrl_file(const char* path, const VrlSet& v, std::string* err)
{
    FILE* f = std::fopen(path, "w");
    if (!f) { *err = std::string("cannot write VRL file ") + path; return false; }
    for (uint32_t i = 0; i < v.n; i++) {
        for (int pl = 0; pl < 9; pl++)
            std::fprintf(f, pl ? " %.9g" : "%.9g", (double)v.soa[(size_t)pl * v.n + i]);
        std::fputc('\n', f);
    }
    std::fclose(f);
    return true;
}

}  // namespace host
}  // namespace alvrl
