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
