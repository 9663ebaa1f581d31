"""CPU: what the read-list ABI (include/iteres_amd.h itx_names_*) answers before it touches a device — bad arguments are error
codes with a message, never a crash."""
import ctypes as C

import pytest

from iteres_amd import build, engine as eng


@pytest.fixture(scope="module")
def lib():
    build.build_lib()
    return eng.load()


def test_bad_arguments_need_no_gpu(lib):
    h = C.c_void_p()
    hard = C.c_uint64()
    res = eng.NamesResult()
    assert lib.itx_names_create(0, 0, 0, C.byref(h)) == -1 and b"itx_names_create" in lib.itx_last_error()
    assert lib.itx_names_create(0, 16, 0, None) == -1
    assert lib.itx_names_create(0, 1 << 33, 0, C.byref(h)) == -1                      # more records than a batch can number
    assert lib.itx_names_finish(None, 1, C.byref(res)) == -1
    assert lib.itx_names_append_host(None, None, None, None, 0) == -1
    assert lib.itx_names_run(None, None, None, None, 0, None, C.byref(hard)) == -1
    assert lib.itx_bamwin_names(None, None, 0, 0, None, None, C.byref(hard)) == -1
    assert lib.itx_names_wait_kernels(None) == -1 and lib.itx_names_get_stats(None, None) == -1
    assert lib.itx_names_hits(None) is None and lib.itx_names_stream(None) is None
    lib.itx_names_destroy(None)


def test_wrapper_structs_match_the_header():
    assert C.sizeof(eng.NamesResult) == 40 and C.sizeof(eng.NamesStats) == 64
