"""The gpuChains property and the statistics' path flags (no GPU needed: the
property parser fails before the integrator opens a device, and the struct
is plain ctypes)."""
import ctypes as C

import pytest


@pytest.fixture(scope="module")
def alvrl():
    import alvrl as a
    return a


def _create_error(alvrl, props):
    """alvrl_integrator_create's error for props, or None if they parse (the
    call may then fail later for want of a device, with another message)."""
    L = alvrl._host()
    h = C.c_void_p()
    rc = L.alvrl_integrator_create(props.encode(), 0, C.byref(h))
    if rc == alvrl.ALVRL_OK:
        L.alvrl_integrator_destroy(h)
        return None
    return L.alvrl_host_last_error().decode()


@pytest.mark.parametrize("value", ["true", "false", "1", "0"])
def test_gpu_chains_is_a_known_boolean(alvrl, value):
    err = _create_error(alvrl, f"gpuChains={value}")
    assert err is None or ("gpuChains" not in err and "unknown" not in err), err


def test_gpu_chains_rejects_other_values_like_other_booleans(alvrl):
    err = _create_error(alvrl, "gpuChains=maybe")
    ref = _create_error(alvrl, "gpuTracer=maybe")
    assert err == "bad boolean for gpuChains: maybe"
    assert ref == "bad boolean for gpuTracer: maybe"


def test_stats_carry_the_path_flags(alvrl):
    names = [n for n, _ in alvrl.IntegratorStats._fields_]
    assert names[-2:] == ["traced_on_device", "chains_on_device"]
    assert names[-3] == "ms_alloc"                                   # grown at the tail only
    st = alvrl.IntegratorStats()
    assert C.sizeof(st) % 8 == 0
    assert set(st.as_dict()) >= {"traced_on_device", "chains_on_device"}
