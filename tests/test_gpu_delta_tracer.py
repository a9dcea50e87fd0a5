"""The device VRL tracer on scenes with delta surfaces: mirrors, a null pane
(test_chains.chain_mesh) and glass (test_dielectric.glass_mesh).

Bar: bit equality.  alvrl.trace_vrls_gpu against the oracle's tracer and the
host tracer (which test_chains.py / test_dielectric.py hold bit-equal to the
oracle): the VRL planes, their number and the particle count, over
short_vrls, the pass, rrDepth and maxParticleDepth; the size query agrees;
and the set differs from the all-diffuse scene's, so a tracer that ignored
the materials could not pass."""
import ctypes as C

import numpy as np
import pytest

from oracle import set_occluders
from test_chains import ALB, SPEC, chain_mesh
from test_dielectric import glass_mesh

pytestmark = pytest.mark.gpu

SEED_VRL = 0x5EED0001
TARGET = 3000
MESHES = {"chain": (chain_mesh, None), "glass1.5": (glass_mesh, 1.5), "glass1.3333": (glass_mesh, 1.3333)}


def _scenes(oracle, name):
    import alvrl
    mesh, eta = MESHES[name]
    tris, mat = mesh()
    s = alvrl.scene_set_occluders(alvrl.scene_default(16, 16), tris, ALB, material=mat, specular=SPEC, eta=eta)
    o = set_occluders(oracle.scene(16, 16), tris, ALB, material=mat, specular=SPEC, eta=eta)
    return s, o, tris


def _size_query(s, **kw):
    import alvrl
    L = alvrl._host()
    n, pc = C.c_uint32(), C.c_uint64()
    alvrl._hcheck(L.alvrl_trace_vrls_gpu(C.byref(s), kw["seed"], kw["pass_"], TARGET, int(kw["short_vrls"]),
                                         kw["max_depth"], kw["rr_depth"], None, 0, C.byref(n), C.byref(pc)))
    return n.value, pc.value


@pytest.mark.parametrize("pass_,rr_depth,max_depth", [(0, 5, -1), (3, 2, -1), (1, 5, 6)])
@pytest.mark.parametrize("short", [True, False])
@pytest.mark.parametrize("name", list(MESHES))
def test_delta_tracer_matches_oracle_and_host(oracle, gpu_ok, name, short, pass_, rr_depth, max_depth):
    import alvrl
    s, o, tris = _scenes(oracle, name)
    kw = dict(seed=SEED_VRL, pass_=pass_, short_vrls=short, max_depth=max_depth, rr_depth=rr_depth)
    dev, dpc = alvrl.trace_vrls_gpu(s, TARGET, **kw)
    ref, rpc = oracle.trace(o, oracle.medium(), TARGET, **kw)
    host, hpc = alvrl.trace_vrls(s, TARGET, **kw)
    assert dev.shape == ref.shape == host.shape and dev.shape[1] >= TARGET
    assert dpc == rpc == hpc
    assert np.array_equal(dev.view(np.uint32), ref.view(np.uint32))
    assert np.array_equal(dev.view(np.uint32), host.view(np.uint32))
    assert _size_query(s, **kw) == (dev.shape[1], dpc)
    # the materials matter: the all-diffuse scene over the same triangles gives another set
    diffuse = alvrl.scene_set_occluders(alvrl.scene_default(16, 16), tris, ALB)
    plain, _ = alvrl.trace_vrls_gpu(diffuse, TARGET, **kw)
    assert plain.shape != dev.shape or not np.array_equal(plain, dev)


def test_delta_tracer_area_emitter(gpu_ok):
    """An area emitter over the mirror / null scene: device == host."""
    import alvrl
    tris, mat = chain_mesh()
    s = alvrl.scene_set_occluders(alvrl.scene_default(16, 16), tris, ALB, material=mat, specular=SPEC)
    em = np.array([[-0.3, 0.9, 0.3, 0.3, 0.9, 0.3, 0.3, 0.9, 0.7],
                   [-0.3, 0.9, 0.3, 0.3, 0.9, 0.7, -0.3, 0.9, 0.7]], np.float32)   # facing down
    alvrl.scene_set_area_emitter(s, em, (5.0, 4.0, 3.0))
    dev, dpc = alvrl.trace_vrls_gpu(s, TARGET, seed=SEED_VRL)
    host, hpc = alvrl.trace_vrls(s, TARGET, seed=SEED_VRL)
    assert dpc == hpc and dev.shape == host.shape and dev.shape[1] >= TARGET
    assert np.array_equal(dev.view(np.uint32), host.view(np.uint32))
