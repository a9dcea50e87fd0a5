"""One integrator whose frame grows between renders, with the eye paths'
chains formed on the device (gpuChains): the record buffer left by the
smaller frame is shorter than the larger frame's primary blocks, behind
which the chain records are written.  Bar: the frame equals, bit for bit,
that of a fresh integrator with gpuChains=false.  And the statistics keep
naming the device path when a render reuses its cached records."""
import numpy as np
import pytest

from test_chains import ALB, SPEC, chain_mesh
from test_dielectric import glass_mesh

pytestmark = pytest.mark.gpu

W, H = 24, 16
SEED = 0xA1B2C3D4
MESHES = {"chain": chain_mesh, "glass": glass_mesh}


def _scene(name, w, h):
    import alvrl
    tris, mat = MESHES[name]()
    return alvrl.scene_set_occluders(alvrl.scene_default(w, h), tris, ALB, material=mat, specular=SPEC, eta=1.5)


def _frame(it, n, **kw):
    import torch
    fb = torch.zeros(n * 3, dtype=torch.float32, device="cuda")
    it.render(fb, **kw)
    torch.cuda.synchronize()
    return fb.cpu().numpy()


def _reference(name, props):
    """The 24x16 frame of pass 1 from a fresh integrator with the host's chains."""
    import alvrl
    it = alvrl.Integrator(props + ";gpuChains=false", device=0)
    try:
        it.preprocess(_scene(name, W, H))
        it.prepass(1)
        return _frame(it, W * H)
    finally:
        it.close()


@pytest.mark.parametrize("name", list(MESHES))
def test_preprocess_again_with_a_larger_frame(gpu_ok, name):
    import alvrl
    props = f"localRefinement=false;globalCluster=false;vrlTargetNum=1000;seed={SEED}"
    it = alvrl.Integrator(props, device=0)
    try:
        it.preprocess(_scene(name, 8, 8))
        it.prepass(0)
        small = _frame(it, 64)
        assert np.isfinite(small).all() and small.max() > 0
        it.preprocess(_scene(name, W, H))
        it.prepass(1)
        big = _frame(it, W * H)
        assert it.stats()["chains_on_device"] == 1
    finally:
        it.close()
    ref = _reference(name, props)
    assert big.max() > 0
    assert np.array_equal(big.view(np.uint32), ref.view(np.uint32))


@pytest.mark.parametrize("name", list(MESHES))
def test_render_an_empty_share_then_the_whole_frame(gpu_ok, name):
    """Rank 1 of 2 owns no tile of a 24x16 frame; the whole frame follows on
    the same integrator (clustered)."""
    import alvrl
    props = f"targetNumSlices=12;vrlTargetNum=1000;seed={SEED}"
    it = alvrl.Integrator(props, device=0)
    try:
        it.preprocess(_scene(name, W, H))
        it.prepass(1)
        none = _frame(it, W * H, rank=1, world=2)
        assert not none.any()
        whole = _frame(it, W * H)
    finally:
        it.close()
    ref = _reference(name, props)
    assert whole.max() > 0
    assert np.array_equal(whole.view(np.uint32), ref.view(np.uint32))


def test_chain_flag_survives_a_cached_render(gpu_ok):
    """prepass, render, the same prepass, render: the second render reuses the
    cached records, which the device formed."""
    import alvrl
    it = alvrl.Integrator(f"localRefinement=false;globalCluster=false;vrlTargetNum=1000;seed={SEED}", device=0)
    try:
        it.preprocess(_scene("glass", W, H))
        for _ in range(2):
            it.prepass(1)
            a = _frame(it, W * H)
            assert it.stats()["chains_on_device"] == 1
        assert a.max() > 0
    finally:
        it.close()
