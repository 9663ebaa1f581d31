"""CPU-side checks of the itx_loci_* boundary (include/iteres_amd.h): what create refuses it refuses before any device work, so
the checks need no GPU. The device route itself: tests/test_gpu_loci.py; the line rule: tests/test_lociline.py."""
import ctypes as C

import numpy as np
import pytest

from iteres_amd import build, engine as eng


@pytest.fixture(scope="module")
def lib():
    build.build_lib()
    return eng.load()


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def test_create_refuses_before_any_device_work(lib):
    rows = eng.make_rows([0, 0], [10, 470_000_000], [20, 470_000_100], [0, 0], [5, 5], [0, 0], [0, 0], [0, 0])
    row_chrom, rank = np.zeros(2, np.uint32), np.zeros(1, np.uint32)
    name, off = np.frombuffer(b"chr1\0", np.uint8).copy(), np.array([0, 4], np.uint64)
    h = C.c_void_p()

    def create(kind=0, n=1, nc=1, rank_=rank, off_=off, out=h, n_rep=1):
        return lib.itx_loci_create(0, kind, _p(rows), _p(row_chrom), n, _p(rank_), nc, _p(name), _p(off_), _p(name), _p(off), n_rep, _p(name), _p(off), 1, _p(name), _p(off), 1,
                                   C.byref(out) if out is not None else None)
    assert create(out=None) == -1 and create(kind=7) == -1 and create(rank_=None) == -1 and create(off_=None) == -1
    assert b"itx_loci_create" in lib.itx_last_error()
    big_rank, big_off = np.zeros(1 << 19, np.uint32), np.zeros((1 << 19) + 1, np.uint64)
    assert create(nc=1 << 19, rank_=big_rank, off_=big_off) == -2            # ITX_E_RANGE: the key holds 2^19 - 1 chromosomes
    assert create(n=2) == -2 and b"bin" in lib.itx_last_error()              # a short row at 470 M: bin 8266 does not fit 13 bits
    assert create(n_rep=0) == -1                                            # a row names a repName the table does not have
    assert create(rank_=np.array([1], np.uint32)) == -1
    assert h.value is None
    res = eng.LociText()
    assert lib.itx_loci_filter_text(None, None, 1, 5, C.byref(res)) == -1 and lib.itx_loci_cpg_text(None, None, None, 0.0, C.byref(res)) == -1
    assert lib.itx_loci_order(None, None, None) == -1
    lib.itx_loci_destroy(None)
