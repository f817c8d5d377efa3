"""Host-side checks of the community order's entry points: what gdd_community_order rejects before it
touches a device, and the drop-in driver's --relabel option. No GPU."""
import ctypes

import pytest


@pytest.fixture(scope="module")
def lib():
    from gdd import _lib
    return _lib.load()


def test_host_rejections(lib):
    buf = (ctypes.c_int32 * 4096)()
    p = ctypes.addressof(buf)
    need = lib.gdd_community_order_ws_bytes(100, 200)
    assert need >= 6 * 4 * 100
    assert lib.gdd_community_order_ws_bytes(0, 0) > 0
    assert lib.gdd_community_order(-1, 0, p, p, 3, p, None, None, p, need, None) == 0x10001
    assert b"community_order" in lib.gdd_last_error()
    assert lib.gdd_community_order(100, -1, p, p, 3, p, None, None, p, need, None) == 0x10001
    assert lib.gdd_community_order(100, 200, p, p, -1, p, None, None, p, need, None) == 0x10001
    assert b"sweeps" in lib.gdd_last_error()
    assert lib.gdd_community_order(100, 200, None, p, 3, p, None, None, p, need, None) == 0x10001
    assert lib.gdd_community_order(100, 200, p, p, 3, p, None, None, p, 64, None) == 0x10002
    assert b"workspace" in lib.gdd_last_error()
    # n = 0 is valid and has nothing to do
    assert lib.gdd_community_order(0, 0, None, None, 3, None, None, None, p, lib.gdd_community_order_ws_bytes(0, 0),
                                   None) == 0


def test_relabel_option_is_absent_by_default():
    """--relabel leaves a default run's printed Namespace as it was; the agent reads it with getattr."""
    from gdd.train_clustgdd_transduct import parser
    assert not hasattr(parser().parse_args([]), "relabel")
    assert parser().parse_args(["--relabel", "community"]).relabel == "community"
    with pytest.raises(SystemExit):
        parser().parse_args(["--relabel", "nope"])
