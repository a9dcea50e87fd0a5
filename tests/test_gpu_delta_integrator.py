"""The integrator on scenes with delta surfaces, device paths on and off.

With the defaults (gpuTracer, gpuChains) the pass's VRLs are traced and the
eye paths' chains are formed on the device; with both off the host does
both.  Bar: bit equality of everything downstream -- the VRLs, R, the cluster
lists and the frame -- over two passes, and the statistics name the path
that ran."""
import numpy as np
import pytest

from test_chains import ALB, SPEC, chain_mesh
from test_dielectric import glass_mesh

pytestmark = pytest.mark.gpu

W, H = 24, 16
SEED = 0xA1B2C3D4
HOST = "gpuTracer=false;gpuChains=false"
MESHES = {"chain": chain_mesh, "glass": glass_mesh}


def _scene(name):
    import alvrl
    tris, mat = MESHES[name]()
    return alvrl.scene_set_occluders(alvrl.scene_default(W, H), tris, ALB, material=mat, specular=SPEC, eta=1.5)


def _run(name, props):
    """Two passes; per pass the frame, the VRLs, R and the cluster lists (the
    last two when the integrator clusters), and the statistics."""
    import torch
    import alvrl
    it = alvrl.Integrator(props + f";vrlTargetNum=2000;seed={SEED}", device=0)
    out = []
    try:
        it.preprocess(_scene(name))
        for p in range(2):
            it.prepass(p)
            fb = torch.zeros(W * H * 3, dtype=torch.float32, device="cuda")
            it.render(fb)
            torch.cuda.synchronize()
            res = {"frame": fb.cpu().numpy(), "vrls": it.vrls()[0], "particles": np.array([it.vrls()[1]])}
            if "localRefinement=false" not in props:
                res["R"] = it.R()
                res.update(it.clusters())
            out.append((res, it.stats()))
    finally:
        it.close()
    return out


@pytest.mark.parametrize("spp", [1, 2])
@pytest.mark.parametrize("props", ["targetNumSlices=12", "localRefinement=false;globalCluster=false"])
@pytest.mark.parametrize("name", list(MESHES))
def test_device_paths_equal_host_paths(gpu_ok, name, props, spp):
    props = f"{props};sampleCount={spp}"
    dev = _run(name, props)
    host = _run(name, props + ";" + HOST)
    for p, ((d, dst), (h, hst)) in enumerate(zip(dev, host)):
        assert d.keys() == h.keys()
        for k in d:
            assert d[k].shape == h[k].shape, (p, k)
            assert np.array_equal(d[k].view(np.uint32), h[k].view(np.uint32)), (p, k)
        assert np.isfinite(d["frame"]).all() and d["frame"].max() > 0
        assert dst["traced_on_device"] == 1 and dst["chains_on_device"] == 1
        assert hst["traced_on_device"] == 0 and hst["chains_on_device"] == 0
    # the passes differ (their VRLs and the chains' roulette): two passes check two things
    assert not np.array_equal(dev[0][0]["vrls"], dev[1][0]["vrls"])


def test_host_cast_scene_traces_delta_scene_on_device(gpu_ok):
    """A host-cast scene whose tracer descriptor has mirrors and a null pane:
    the pass's VRLs are the same with gpuTracer on and off."""
    import alvrl
    s = _scene("chain")
    tris, mat = chain_mesh()
    sr = np.stack([alvrl.scene_slice_record(s, x, y) for y in range(H) for x in range(W)])
    got = []
    for extra, on in (("", 1), (";gpuTracer=false", 0)):
        it = alvrl.Integrator(f"localRefinement=false;globalCluster=false;vrlTargetNum=2000;seed={SEED}" + extra, device=0)
        try:
            it.preprocess_ext(W, H, sr, list(s.box_min), list(s.box_max), alvrl.Medium(), tris, mat, tracer=s)
            it.prepass(1)
            got.append(it.vrls())
            assert it.stats()["traced_on_device"] == on
        finally:
            it.close()
    (a, pa), (b, pb) = got
    assert pa == pb and a.shape == b.shape and a.shape[1] >= 2000
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
