// scene.hpp -- standalone smoke-box scene: the minimal stand-in for the parts
// of Mitsuba's Scene / Sensor / Shape / Emitter that the vrl integrator calls
// (out of scope per SURVEY.md 2; restated only as far as the benchmark scene
// needs them):
//   perspective pinhole  src/sensors/perspective.cpp:126-155, 247-269
//   ray / box walls      one-sided diffuse walls of an axis-aligned box, seen
//                        from inside
//   occluders            optional triangles inside the box (a TriMesh with a
//                        one-sided diffuse BSDF): TriangleT::rayIntersect
//                        (include/mitsuba/core/triangle.h:109-145), the hit
//                        record of skdtree.h:350-396, and the visibility
//                        part of Scene::evalTransmittance (scene.cpp:619-679);
//                        without them every interior pair is mutually visible
//   point light          src/emitters/point.cpp:81-106
//   homogeneous fog      src/medium/homogeneous.cpp (balance / single /
//                        manual / maximum distance sampling)
#pragma once

#include <cstdint>
#include <string>
#include <vector>

#include "../transport.h"

namespace alvrl {
namespace host {

// the vector (host::V3), the medium and the walks are the shared ones (csrc/transport.h)
using transport::Camera;
using transport::kRecWords;
using transport::MediumParams;
using transport::SceneView;
using transport::V3;
using transport::v3;

// A SmokeBox as the shared walks see it, with the occluder query of the host:
// every triangle in index order.
struct HostScene : SceneView {
    const float* occ;
    uint32_t nocc;
    const float* closest_occluder(V3 o, V3 d, float mint, float* best, int* id, float* bu, float* bv) const
    {
        for (uint32_t i = 0; i < nocc; i++) {   // shape kd-tree leaf test, t in [mint, maxt] (skdtree.h:248-262)
            float u, v, t;
            if (!tri_intersect(occ + 9 * (size_t)i, o, d, &u, &v, &t)) continue;
            if (t < mint || !(t < *best)) continue;
            *best = t; *id = (int)i; *bu = u; *bv = v;
        }
        return occ + 9 * (size_t)(*id < 0 ? 0 : *id);
    }
};

struct SmokeBox {
    V3 cam_origin = v3(0.0f, 0.0f, -0.9f);
    V3 cam_target = v3(0.0f, 0.0f, 1.0f);
    V3 cam_up = v3(0.0f, 1.0f, 0.0f);
    float fov_x_deg = 60.0f;
    int width = 1024, height = 1024;
    float box_min[3] = {-1.0f, -1.0f, -1.0f};
    float box_max[3] = {1.0f, 1.0f, 1.0f};
    float albedo[3] = {0.5f, 0.5f, 0.5f};
    V3 light_pos = v3(0.0f, 0.8f, 0.0f);
    float light_intensity[3] = {10.0f, 10.0f, 10.0f};
    MediumParams medium;
    std::vector<float> occ;           // occluder triangles, 9 floats each (p0, p1, p2)
    float occ_albedo[3] = {0.5f, 0.5f, 0.5f};
    std::vector<float> occ_alb;       // per triangle reflectance, 3 floats each (empty: occ_albedo for all)
    std::vector<uint32_t> occ_mat;    // per triangle ALVRL_MAT_* (empty: all diffuse)
    float occ_spec[3] = {1.0f, 1.0f, 1.0f};
    // dielectric triangles: m_eta = intIOR / extIOR (dielectric.cpp:149-158; bk7 / air, ior.h:43, 60)
    float occ_eta = 1.5046f / 1.000277f;
    // area emitter (alvrl_scene_desc::emitter_tris): triangles, radiance, and
    // TriMesh's sampling table (prepare_emitter): the normalized area CDF of
    // DiscreteDistribution (pmf.h:101-114) and the surface area
    std::vector<float> emit;
    float emit_radiance[3] = {0.0f, 0.0f, 0.0f};
    std::vector<float> emit_cdf;
    float emit_area = 0.0f;
    bool area_light() const { return !emit.empty(); }
    void prepare_emitter();
    bool has_delta() const
    {
        for (uint32_t m : occ_mat) if (m != 0u) return true;
        return false;
    }
    uint32_t n_occ() const { return (uint32_t)(occ.size() / 9); }

    // the scene and the camera's per-scene terms (perspective.cpp:126-155) as
    // the shared walks read them; the view points into this SmokeBox
    HostScene view() const;
    Camera camera() const;
    // The eye path of sensor sample j of spp of pixel (x, y) through delta
    // BSDFs (chain_walk, transport.h), record 0 included.  Appends kRecWords
    // floats per record (<= 256).
    void make_chain(int x, int y, bool medium_scatters, uint32_t seed, uint32_t pass, int spec_rr_depth,
                    float init_throughput, std::vector<float>* out, uint32_t sample = 0, uint32_t spp = 1) const;
    // buildSlices' gather point of pixel (x, y) (Preprocessor.cpp:1144-1170):
    // the camera ray's first hit, continued through null surfaces; a record
    // with the hit flag, position and normal of that point.
    void make_slice_record(int x, int y, float rec[kRecWords]) const;
    // Gather record (alvrl_gather_rec layout) of pixel centre (x, y), or of
    // its sensor sample j of spp; the depth word carries j in bits 16-31.
    void make_record(int x, int y, bool medium_scatters, float rec[kRecWords], uint32_t seed = 0,
                     uint32_t pass = 0, uint32_t sample = 0, uint32_t spp = 1) const;
    float scene_diagonal() const;   // distance(getAABB().min, getAABB().max)
};

// vrlVector: SoA planes (start xyz, end xyz, power rgb), VRL.h:105-194.
struct VrlSet {
    std::vector<float> soa;   // 9 * n, plane stride n
    uint32_t n = 0;
    uint64_t particle_count = 0;
};

// vrlTracer::randomWalk (vrlTracer.h:13-230) in the smoke box, with the
// counter-based stream (seed, pass, particle index) instead of one sequential
// sampler, so the VRL set does not depend on how particles are scheduled.
VrlSet trace_vrls(const SmokeBox& s, uint32_t seed, uint32_t pass, uint32_t target, bool short_vrls,
                  int max_depth, int rr_depth);

// ASCII VRL file I/O: one VRL per line "sx sy sz ex ey ez r g b"
// (VRL.h:43-54 reader, vrlVector(Stream*, Medium*) :120-128).  particleCount =
// number of lines that pass the put-filter.  The writer separates fields with
// spaces (the reference's serializeAscii, VRL.h:65-73, writes none and cannot
// be read back).
bool read_vrl_file(const char* path, const MediumParams& m, VrlSet* out, std::string* err);
bool write_vrl_file(const char* path, const VrlSet& v, std::string* err);

}  // namespace host
}  // namespace alvrl
