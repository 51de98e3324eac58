"""Every row of tests/api_cases.py through the real library: the status and the tn_last_error text of each device entry point.

A row that the library must refuse goes to the CPU stepping of the same checks first (emu_api_check runs the list capi.cpp runs),
so a check that no longer refuses is found before a pointer of that row reaches the device.  Rows that are accepted run on
buffers of one arena that is large enough for every one of them."""
import pytest

import api_cases
import emu_library
from api_cases import FUSED, GENERAL, NULL, OK, OMEGA
from conftest import PARAMS

pytestmark = pytest.mark.gpu

BATCH, TERMS = 5, 2
ENTRIES = sorted({c.entry for c in api_cases.cases(BATCH, TERMS, 60)})


@pytest.fixture(scope="module")
def eng():
    import torch
    assert torch.cuda.is_available()
    from tiny_ntt_amd import engine
    return engine


@pytest.fixture(scope="module")
def arenas(eng):
    made = {}

    def get(tag):
        if tag not in made:
            n, q, psi = PARAMS[tag]
            plans = {FUSED: eng.get_plan(n, q, psi), GENERAL: eng.get_general_plan(n, q, psi), OMEGA: eng.get_omega_plan(n, q, pow(psi, 2, q))}
            assert plans[FUSED].has_fused and not plans[GENERAL].has_fused and not plans[OMEGA].has_fused
            made[tag] = plans, plans[FUSED].fill_lcg(api_cases.ARENA_ROWS, 1, 2)            # canonical words everywhere
        return made[tag]
    return get


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("tag", ["P256", "P4096_60"])
def test_every_row_of_the_table_gives_its_status_and_text(eng, arenas, tag, entry):
    import torch
    n, q, psi = PARAMS[tag]
    plans, arena = arenas(tag)
    plan = plans[FUSED]
    lib, emu = plan._lib, emu_library.load()
    stream = plan._stream_ptr(None)
    row_bytes = n * plan.elem_bytes
    assert arena.shape == (api_cases.ARENA_ROWS, n) and arena.element_size() == plan.elem_bytes and arena.is_contiguous()
    wrong = []
    for c in (c for c in api_cases.cases(BATCH, TERMS, q.bit_length()) if c.entry == entry):
        if c.status != OK:
            assert api_cases.emu_case(emu, c, n, plan.elem_bytes, q, arena.data_ptr())[0] == c.status, c.id
        handle = None if c.plan == NULL else plans[c.plan]._h
        st = getattr(lib, entry)(handle, *api_cases.c_arguments(c, arena.data_ptr(), row_bytes), stream)
        text = lib.tn_last_error().decode()
        if st != c.status or (c.text is not None and text != c.text):
            wrong.append((c.id, st, text))
    torch.cuda.synchronize()
    assert not wrong, wrong
