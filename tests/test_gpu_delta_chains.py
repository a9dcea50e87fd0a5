"""The device eye paths on scenes with delta surfaces: the primary records of
alvrl_scene_records_spp_gpu and the chain / tree records of
alvrl_scene_chains_gpu against the host's (alvrl_scene_records_spp,
alvrl_scene_chain_spp -- bit-equal to the oracle, test_chains.py and
test_dielectric.py).

Bar: bit equality of every record's 80 bytes, of the per-pixel counts, the
level grouping (level d = the records of pre-order index d + 1), the pixel
order within a level and the source indices; at the 256-record cap, and with
the pending-sibling stack forced to overflow into the host completion."""
import numpy as np
import pytest

from oracle import set_occluders
from test_chains import ALB, SPEC, chain_mesh
from test_dielectric import glass_mesh

pytestmark = pytest.mark.gpu

SEED = 0xA1B2C3D4
W, H = 24, 16
MESHES = {"chain": chain_mesh, "glass": glass_mesh}


def _scene(name, eta=1.5):
    import alvrl
    tris, mat = MESHES[name]()
    return alvrl.scene_set_occluders(alvrl.scene_default(W, H), tris, ALB, material=mat, specular=SPEC, eta=eta)


def _host_chains(s, pix, **kw):
    """The host's eye path of every pixel, and from them what the device
    entry point must return: counts, level offsets, records, sources."""
    import alvrl
    kw = dict(kw)
    sample, spp = kw.pop("sample", 0), kw.pop("spp", 1)
    chains = [alvrl.scene_chain_spp(s, int(p % W), int(p // W), sample, spp, **kw) for p in pix]
    counts = np.array([len(c) for c in chains], np.uint32)
    recs, src, off = [], [], [0]
    for d in range(1, int(counts.max()) if len(counts) else 0):
        for i, c in enumerate(chains):
            if len(c) > d:
                recs.append(c[d])
                src.append(i)
        off.append(len(recs))
    recs = np.asarray(recs, np.float32).reshape(-1, 20)
    return chains, counts, np.asarray(off, np.uint32), recs, np.asarray(src, np.uint32)


def _assert_same(dev, counts, off, recs, src):
    assert np.array_equal(dev["counts"], counts)
    assert np.array_equal(dev["level_off"], off)
    assert dev["recs"].shape == recs.shape
    assert np.array_equal(dev["recs"].view(np.uint32), recs.view(np.uint32))
    assert np.array_equal(dev["src"], src)
    # the depth word is the pre-order index: level d holds index d + 1
    for d in range(len(off) - 1):
        assert np.all((dev["recs"][off[d]:off[d + 1], 19].view(np.uint32) & 0xFFFF) == d + 1)


@pytest.mark.parametrize("spp", [1, 3])
@pytest.mark.parametrize("name", list(MESHES))
def test_primary_records_match_host(gpu_ok, name, spp):
    import alvrl
    s = _scene(name)
    host = alvrl.scene_records_spp(s, spp, seed=SEED, pass_=2)
    dev = alvrl.scene_records_spp_gpu(s, spp, seed=SEED, pass_=2).cpu().numpy()
    assert host.shape == dev.shape == (spp * W * H, 20)
    assert np.array_equal(dev.view(np.uint32), host.view(np.uint32))
    assert ((host[:, 15].view(np.uint32) & 8) != 0).sum() > 20   # delta first hits are there


@pytest.mark.parametrize("rr_depth,pass_", [(100, 0), (2, 3)])
@pytest.mark.parametrize("name", list(MESHES))
def test_chains_match_host(gpu_ok, name, rr_depth, pass_):
    import alvrl
    s = _scene(name)
    pix = np.arange(W * H, dtype=np.uint32)
    kw = dict(seed=SEED, pass_=pass_, spec_rr_depth=rr_depth)
    _, counts, off, recs, src = _host_chains(s, pix, **kw)
    assert counts.max() >= 4 and len(recs) > 100
    dev = alvrl.scene_chains_gpu(s, **kw)
    _assert_same(dev, counts, off, recs, src)


def test_chains_sample_of_spp(gpu_ok):
    import alvrl
    s = _scene("glass")
    pix = np.arange(W * H, dtype=np.uint32)
    kw = dict(seed=SEED, pass_=1, sample=2, spp=3)
    _, counts, off, recs, src = _host_chains(s, pix, **kw)
    assert len(recs) > 100
    dev = alvrl.scene_chains_gpu(s, **kw)
    _assert_same(dev, counts, off, recs, src)
    assert np.all(dev["recs"][:, 19].view(np.uint32) >> 16 == 2)


def test_chains_without_medium_scatter_and_pixel_list(gpu_ok):
    import alvrl
    s = _scene("chain")
    pix = np.arange(W * H - 1, -1, -3, dtype=np.uint32)            # a descending list: its order is kept
    kw = dict(seed=SEED, medium_scatters=False)
    _, counts, off, recs, src = _host_chains(s, pix, **kw)
    assert len(recs) > 30
    dev = alvrl.scene_chains_gpu(s, pixel_ids=pix, **kw)
    _assert_same(dev, counts, off, recs, src)
    assert not np.any(dev["recs"][:, 15].view(np.uint32) & 4)


def test_chains_match_oracle(oracle, gpu_ok):
    """A few pixels straight against the oracle's own chain."""
    import alvrl
    tris, mat = glass_mesh()
    s = _scene("glass")
    o = set_occluders(oracle.scene(W, H), tris, ALB, material=mat, specular=SPEC, eta=1.5)
    pix = np.arange(5, W * H, 37, dtype=np.uint32)
    dev = alvrl.scene_chains_gpu(s, pixel_ids=pix, seed=SEED, pass_=3, spec_rr_depth=2)
    got = 0
    for i, p in enumerate(pix):
        ref = oracle.chain(o, oracle.medium(), int(p % W), int(p // W), seed=SEED, pass_=3, spec_rr_depth=2)
        assert dev["counts"][i] == len(ref)
        for k in range(1, len(ref)):
            lvl = dev["recs"][dev["level_off"][k - 1]:dev["level_off"][k]]
            row = lvl[dev["src"][dev["level_off"][k - 1]:dev["level_off"][k]] == i]
            assert row.shape == (1, 20) and np.array_equal(row[0].view(np.uint32), ref[k].view(np.uint32))
            got += 1
    assert got > 10


@pytest.fixture(scope="module")
def deep():
    """Glass without roulette: trees that run into the 256-record cap.  The
    host reference, computed once."""
    s = _scene("glass")
    kw = dict(seed=SEED, pass_=0, init_throughput=1e30, spec_rr_depth=1000)
    ref = _host_chains(s, np.arange(W * H, dtype=np.uint32), **kw)
    return s, kw, ref


def test_deep_trees_and_record_cap(gpu_ok, deep):
    import alvrl
    s, kw, (_, counts, off, recs, src) = deep
    assert (counts == 256).sum() >= 1 and counts.max() == 256     # not vacuous: the cap is reached
    assert int(counts.sum()) > 10000
    dev = alvrl.scene_chains_gpu(s, **kw)
    _assert_same(dev, counts, off, recs, src)


def test_forced_stack_overflow_is_completed_by_the_host(gpu_ok, deep):
    import alvrl
    s, kw, (_, counts, off, recs, src) = deep
    dev = alvrl.scene_chains_gpu(s, stack_cap=1, **kw)
    assert dev["overflow"] > 0
    _assert_same(dev, counts, off, recs, src)
