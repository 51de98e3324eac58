"""The one library of the CPU stepping (tests/emu/_build/libemu.so), brought up to date and opened once per process."""
import ctypes
import functools
import os

from conftest import ROOT, _make


@functools.lru_cache(maxsize=None)
def load():
    """make -C tests/emu (nothing to do when the library is newer than its sources and headers), then the ctypes handle."""
    _make("tests/emu")
    return ctypes.CDLL(os.path.join(ROOT, "tests", "emu", "_build", "libemu.so"))


def api_check(entry, *args):
    """An *_api_check entry point of the library on args, whose last three parameters are (int* launch, char* msg, size_t msg_len)
    -> (status, the text tn_last_error would give, the call goes on to a launch)."""
    msg, launch = ctypes.create_string_buffer(256), ctypes.c_int(-1)
    st = entry(*args, ctypes.byref(launch), msg, 256)
    return st, msg.value.decode(), bool(launch.value)


def smallest_dynamic_batch(row_bytes, resident, which=0):
    """The smallest batch that launch_plan.h's plan_rows hands out through the device counter for rows of row_bytes when
    `resident` workgroups are resident (which: 0 the fused kernels' policy, 1 the constant-geometry kernels'); one row fewer keeps
    the fixed stride.  The GPU tests of the dynamic hand-out size their batches with it."""
    L = load()
    sz, ci = ctypes.c_size_t, ctypes.c_int
    L.emu_plan_rows.argtypes = [ci, sz, sz, sz, ctypes.POINTER(ctypes.c_uint32)]
    L.emu_row_policy.argtypes = [ci, ci]; L.emu_row_policy.restype = ctypes.c_long
    chunk = ctypes.c_uint32()
    want = max(1, -(-L.emu_row_policy(which, 0) // row_bytes))
    rows = L.emu_row_policy(which, 1) * resident * want
    assert L.emu_plan_rows(which, row_bytes, rows, resident, ctypes.byref(chunk)) == 1 and chunk.value == want
    assert L.emu_plan_rows(which, row_bytes, rows - 1, resident, ctypes.byref(chunk)) == 0
    return rows
