"""k_stream on inputs built to land on every threshold of its tile routes (streamtiles.py), against the oracle, bit for bit.

Every test first re-asserts the tile classes its input promises (the model's count of tiles with nb == 64 / 65 / 128 / 129,
wn == 128 / 129, records with b == 64, hits at window entry 128, ...), then runs the engine and the oracle on it: stat on the
atomics and on the partition path, filter mode (the per-locus runs), a veto callable (the classify-only launch), and the
first-hit lookup of the cpg commands against binKeeperFind for EVERY record. All comparisons are exact.
"""
import time

import numpy as np
import pytest

import enginecase as ec
import streamtiles as stl
from iteres_amd import engine as eng

pytestmark = pytest.mark.gpu

BUILDERS = {
    "slice_width": stl.build_slice_width,
    "window_size": stl.build_window_size,
    "hit_counts": stl.build_hit_counts,
    "record_route": stl.build_record_route,
    "paired": stl.build_paired,
    "locus_runs": stl.build_locus_runs,
}
NAMES = sorted(BUILDERS)
ACCUMS = [eng.ACCUM_ATOMIC, eng.ACCUM_PARTITION]
CAP = 1 << 16
E0 = dict(extension=0, min_cov=0.0001)
_cache = {}


def _case(name):
    """The builder's input with its promised classes re-asserted, and the table's bin width as the model assumed it."""
    if name not in _cache:
        case = BUILDERS[name]()
        stl.check_promises(case, CAP)
        rows = _rows(case)
        t = eng.Table(rows, case.chrom_size, case.rep_len, case.n_fam, case.n_cla)
        shift = int(t.info.bin_shift)
        t.close()
        _cache[name] = (case, rows, shift)
    case, rows, shift = _cache[name]
    assert shift == stl.SHIFT
    return case, rows


def _rows(case):
    r = case.rows
    return eng.make_rows(r["chrom"], r["start"], r["end"], r["cons_start"], r["cons_end"], r["rep"], r["fam"], r["cla"])


def _both(case, rows, params, accum, cap=CAP, veto=None):
    eres, ores, hits = ec.run_both(rows, case.chrom_size, case.rep_len, case.n_fam, case.n_cla, params, case.tid2chrom, case.rd,
                                   batch_capacity=cap, accum=accum, veto=veto)
    ec.assert_same(eres, ores, hits, bool(params.get("filter_mode")), len(rows))
    return ores


def _veto(h):
    return (h >= 0) & (h % 3 == 0)


def _first_hits(case, rows, cap=CAP):
    """Engine.first_hits_host on the records' plain intervals against the first row binKeeperFind returns, for every record."""
    ot = ec.oracle_table(rows, case.chrom_size, case.rep_len, case.n_fam, case.n_cla)
    t = eng.Table(rows, case.chrom_size, case.rep_len, case.n_fam, case.n_cla)
    e = eng.Engine(t, dict(), batch_capacity=cap)
    e.set_tidmap(case.tid2chrom)
    rd = case.rd
    got = e.first_hits_host(rd["tid"], rd["pos"], rd["tmpend"])
    e.close()
    t.close()
    t2c = case.tid2chrom
    want = np.full(case.n, -1, np.int64)
    for i in range(case.n):
        c = int(t2c[rd["tid"][i]]) if 0 <= rd["tid"][i] < len(t2c) else -1
        if c >= 0:
            h = ot.find(c, int(rd["pos"][i]), int(rd["tmpend"][i]), cap=8)
            if len(h):
                want[i] = int(h[0])
    ot.close()
    bad = np.flatnonzero(got.astype(np.int64) != want)
    assert len(bad) == 0, (case.name, len(bad), bad[:8], got[bad[:8]], want[bad[:8]])
    return want


@pytest.mark.parametrize("accum", ACCUMS)
@pytest.mark.parametrize("name", NAMES)
def test_stat(name, accum):
    case, rows = _case(name)
    ores = _both(case, rows, E0, accum)
    if name != "record_route":
        assert (ores["hit_row"] >= 0).mean() > 0.2


@pytest.mark.parametrize("accum", ACCUMS)
@pytest.mark.parametrize("name", NAMES)
def test_filter_mode(name, accum):
    """ITX_DO_ATOMIC_LOCUS: one atomic per run of equal rows over the lanes (wave_run); builder locus_runs exists for it."""
    case, rows = _case(name)
    ores = _both(case, rows, dict(E0, filter_mode=True), accum)
    assert int(ores["locus_cnt"].sum()) == int(ores["cnt"][9]) > 0


@pytest.mark.parametrize("name", NAMES)
def test_veto(name):
    """ITX_DO_CLASSIFY, then the counting launch over the records the veto left."""
    case, rows = _case(name)
    for accum in ACCUMS:
        _both(case, rows, E0, accum, veto=_veto)


@pytest.mark.parametrize("name", NAMES)
def test_first_hit(name):
    """ITX_DO_FIND_FIRST walks the same tiles, slices and windows."""
    case, rows = _case(name)
    want = _first_hits(case, rows)
    assert (want >= 0).sum() > 100


@pytest.mark.parametrize("min_cov", [0.25, 0.5])
@pytest.mark.parametrize("name", ["slice_width", "window_size", "hit_counts"])
def test_extension_and_min_cov(name, min_cov):
    """-E 150 stretches every read over more bins and rows (the model's classes need not hold), -c 0.25 / 0.5 cuts among them."""
    case, rows = _case(name)
    for accum in ACCUMS:
        ores = _both(case, rows, dict(extension=150, min_cov=min_cov), accum)
    assert 0 < (ores["hit_row"] >= 0).sum() < case.n


@pytest.mark.parametrize("cap", [1024, 1025, 7001])
@pytest.mark.parametrize("tail", [1, 255, 256, 257, 1023])
def test_tails_and_cuts(tail, cap):
    """Ragged last tiles (n mod 1024) and batch ends on and inside tiles. The first-hit lookup and the veto run at the capacity
    off the tile only (7001), and the first-hit lookup not under ITX_STREAM_BLOCKS (test_counter_spills): it writes no counters,
    and its tiles, tails and cuts are those of the launches compared here."""
    key = ("tails", tail)
    if key not in _cache:
        case = stl.build_tails(8 * 1024 + tail)
        _cache[key] = (case, _rows(case))
    case, rows = _cache[key]
    K = stl.classes(case, cap)
    assert K["n_mod_1024"] == tail and (K["batch_end_inside_tile"] > 0) == (cap % 256 != 0)
    assert K["ragged_tiles"] >= (1 if tail % 256 or cap % 256 else 0)
    for accum in ACCUMS:
        _both(case, rows, E0, accum, cap=cap)
    _both(case, rows, dict(E0, filter_mode=True), eng.ACCUM_ATOMIC, cap=cap)
    if cap == 7001:
        _both(case, rows, E0, eng.ACCUM_ATOMIC, cap=cap, veto=_veto)
        _first_hits(case, rows, cap=cap)


@pytest.mark.parametrize("blocks", ["1", "3"])
def test_counter_spills(blocks, monkeypatch):
    """cnt[0..7] sit in 6-bit fields spilled every 15 tiles: one launch in which every wave walks at least 31 tiles of records
    that all count (two spills and a remainder), over one and over three workgroups."""
    if "spill" not in _cache:
        case = stl.build_tails(stl.SPILL_N)
        _cache["spill"] = (case, _rows(case))
    case, rows = _cache["spill"]
    assert stl.tiles_per_wave(case.n, int(blocks)) >= 31
    assert ((case.rd["flag"] & 4) == 0).mean() > 0.9
    monkeypatch.setenv("ITX_STREAM_BLOCKS", blocks)
    for accum in ACCUMS:
        _both(case, rows, E0, accum, cap=case.n)
    _both(case, rows, dict(E0, filter_mode=True), eng.ACCUM_ATOMIC, cap=case.n)
    _both(case, rows, E0, eng.ACCUM_ATOMIC, cap=case.n, veto=_veto)


def test_counter_limit(monkeypatch):
    """The width of the 16-bit halves the 6-bit fields spill into: 16000 * 1024 mapped, unique, classified single-end records
    through ONE workgroup (the longest span itx_launch_stream admits), every lane adding 4 to the same counters in every tile.
    One record more in the batch must give the right sums too or be refused; never wrong counts."""
    monkeypatch.setenv("ITX_STREAM_BLOCKS", "1")
    n = 16000 * stl.WG_TILE
    assert stl.tiles_per_wave(n, 1) == 16000
    rows = eng.make_rows([0], [100], [300], [0], [400], [0], [0], [0])
    rl = np.array([400], np.uint32)
    for m in (n, n + 1):
        rd = {"tid": np.zeros(m, np.int32), "pos": np.full(m, 150, np.int32), "tmpend": np.full(m, 160, np.int32),
              "mapq": np.full(m, 40, np.uint8), "flag": np.zeros(m, np.uint16), "mpos": np.zeros(m, np.int32), "isize": np.zeros(m, np.int32)}
        t0 = time.time()
        ot = ec.oracle_table(rows, [10_000], rl, 1, 1)
        ores = ot.run(E0, [0], rd["tid"], rd["pos"], rd["tmpend"], rd["mapq"], rd["flag"])
        ot.close()
        t = eng.Table(rows, [10_000], rl, 1, 1)
        e = eng.Engine(t, dict(E0, accum=eng.ACCUM_ATOMIC), batch_capacity=m)      # the staging slots: closed on either outcome
        try:
            e.set_tidmap([0])
            try:
                hits = e.submit_host(rd["tid"], rd["pos"], rd["tmpend"], rd["mapq"], eng.flag5(rd["flag"]), want_hits=True)
            except eng.ItxError as err:
                # the only refusal meant here is itx_launch_stream's check of the span, not an allocation or an argument
                assert m > n, f"the longest admitted span was refused: {err}"
                assert "span" in str(err), err
                continue
            eres = e.finish()
        finally:
            e.close()
            t.close()
        print(f"counter limit: {m} records, engine and oracle in {time.time() - t0:.1f} s")
        ec.assert_same(eres, ores, hits, False, 1)
        assert int(eres["cnt"][0]) == int(eres["cnt"][6]) == int(eres["cnt"][7]) == int(eres["cnt"][9]) == int(eres["cnt"][10]) == m
        assert int(eres["rep_cnt"][0]) == m and int(eres["cov"][50:60].min()) == m == int(eres["cov"].max())
