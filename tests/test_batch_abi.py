"""The batch entry points (gprhip_batch_*) are declared, exported and bound, and fail loudly without a device."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BATCH_SYMBOLS = ("gprhip_batch_create", "gprhip_batch_destroy", "gprhip_batch_lanes", "gprhip_batch_lane", "gprhip_batch_eval")


def _header():
    return open(os.path.join(ROOT, "include", "gprhip.h")).read()


def test_batch_symbols_are_declared_exported_and_bound():
    from gpr_amd import _lib
    code = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in BATCH_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, code), "include/gprhip.h does not declare %s" % name
        assert hasattr(lib, name), "libgprhip.so does not export %s" % name
        assert name in _lib.SIGNATURES, "gpr_amd/_lib.py does not bind %s" % name


def test_max_batch_is_the_same_in_header_and_mirror():
    from gpr_amd import _lib
    m = re.search(r"#define\s+GPRHIP_MAX_BATCH\s+(\d+)", _header())
    assert m and int(m.group(1)) == _lib.MAX_BATCH == 64


def test_batch_create_without_a_device_is_a_hip_error(gpu_available):
    """No CPU fallback: without a device the creation fails with GPRHIP_EHIP before it looks at its arguments; with one,
    the missing problem is a bad argument.  Either way nothing is created."""
    from gpr_amd import _lib
    lib = _lib.load()
    h = ctypes.c_void_p()
    st = lib.gprhip_batch_create(None, 2, ctypes.byref(h))
    assert st == (_lib.EBADARG if gpu_available else _lib.EHIP), (st, lib.gprhip_last_error())
    assert not h.value and lib.gprhip_last_error()
    assert lib.gprhip_batch_lanes(None) == 0 and not lib.gprhip_batch_lane(None, 0)
    lib.gprhip_batch_destroy(None)
