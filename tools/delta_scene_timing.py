#!/usr/bin/env python3
"""What a pass costs on a scene with delta surfaces.

Renders the mirror / null scene (tests/test_chains.py chain_mesh) and the
glass scene (tests/test_dielectric.py glass_mesh) with the integrator at
1024 x 1024, 100k VRLs, targetNumSlices=100, sampleCount=1, for three passes,
and prints per pass the tracer's time (ms_trace), the prepass's wall time
(ms_prepass_wall: tracer, R build with the rows' eye paths, clustering), the
wall time of render (the frame's eye paths and the gather, to a device
synchronise) and the statistics' path flags.  The first pass is the warm-up
(code objects, allocations); "steady" is the median of the others.  A
checksum of every pass's frame and VRL set lets two libraries be compared on
results as well as on time.

To time another build of the library (the parent commit's, say) with the same
script, point ALVRL_LIB at its libalvrl.so:

    ALVRL_LIB=/path/to/parent/libalvrl.so python tools/delta_scene_timing.py --label parent
    python tools/delta_scene_timing.py --props "gpuChains=false"

One JSON object per line: {"scene", "pass", ...} per pass, then {"scene",
"steady": {...}} per scene."""
import argparse
import hashlib
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("tests", "oracle", "mitsuba-alvrl_amd"):
    sys.path.insert(0, os.path.join(REPO, p))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--vrls", type=int, default=100000)
    ap.add_argument("--slices", type=int, default=100)
    ap.add_argument("--spp", type=int, default=1)
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--props", default="", help="further integrator properties, e.g. gpuChains=false")
    ap.add_argument("--scenes", default="chain,glass")
    ap.add_argument("--out", default="", help="also append the lines to this file")
    ap.add_argument("--label", default="", help="names the build in the header line (e.g. parent)")
    a = ap.parse_args()

    import numpy as np
    import torch
    import alvrl
    from test_chains import ALB, SPEC, chain_mesh
    from test_dielectric import glass_mesh

    if not torch.cuda.is_available():
        sys.exit("delta_scene_timing.py measures on the GPU: no HIP device is visible")
    meshes = {"chain": chain_mesh, "glass": glass_mesh}
    sink = open(a.out, "a") if a.out else None

    def emit(obj):
        line = json.dumps(obj)
        print(line, flush=True)
        if sink:
            sink.write(line + "\n")
            sink.flush()

    emit({"label": a.label, "library": os.path.basename(alvrl.LIB_PATH), "size": a.size, "vrls": a.vrls, "slices": a.slices, "spp": a.spp,
          "props": a.props, "device": torch.cuda.get_device_name(0)})
    for name in a.scenes.split(","):
        tris, mat = meshes[name]()
        s = alvrl.scene_set_occluders(alvrl.scene_default(a.size, a.size), tris, ALB, material=mat, specular=SPEC,
                                      eta=1.5)
        props = f"targetNumSlices={a.slices};sampleCount={a.spp};vrlTargetNum={a.vrls}"
        it = alvrl.Integrator(props + (";" + a.props if a.props else ""), device=0)
        rows = []
        try:
            t0 = time.perf_counter()
            it.preprocess(s)
            emit({"scene": name, "ms_preprocess_wall": (time.perf_counter() - t0) * 1e3})
            fb = torch.zeros(a.size * a.size * 3, dtype=torch.float32, device="cuda")
            for p in range(a.passes):
                it.prepass(p)
                fb.zero_()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                it.render(fb)
                torch.cuda.synchronize()
                ms_render = (time.perf_counter() - t0) * 1e3
                st = it.stats()
                row = {"scene": name, "pass": p, "ms_trace": st["ms_trace"], "ms_prepass_wall": st["ms_prepass_wall"],
                       "ms_render_wall": ms_render, "ms_render_kernel": st["ms_render_kernel"],
                       "ms_rbuild": st["ms_rbuild"], "vrls": st["vrls"],
                       "traced_on_device": st.get("traced_on_device", 0),
                       "chains_on_device": st.get("chains_on_device", 0),
                       "frame_sha1": hashlib.sha1(fb.cpu().numpy().tobytes()).hexdigest()[:16],
                       "vrls_sha1": hashlib.sha1(np.ascontiguousarray(it.vrls()[0]).tobytes()).hexdigest()[:16]}
                rows.append(row)
                emit(row)
        finally:
            it.close()
        rest = rows[1:] or rows
        emit({"scene": name, "steady": {k: statistics.median(r[k] for r in rest)
                                        for k in ("ms_trace", "ms_prepass_wall", "ms_render_wall", "ms_render_kernel")},
              "passes_in_median": len(rest)})
    if sink:
        sink.close()


if __name__ == "__main__":
    main()
