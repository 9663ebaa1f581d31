"""The tile model of streamtiles.py, proved without the engine: every builder's input lands on the tile classes it promises,
and the model's hit lists (which rows a record overlaps, in binKeeperFind's list order) equal the oracle's for every record."""
import numpy as np
import pytest

import streamtiles as stl
from oracle import binding as orc

BUILDERS = {
    "slice_width": stl.build_slice_width,
    "window_size": stl.build_window_size,
    "hit_counts": stl.build_hit_counts,
    "record_route": stl.build_record_route,
    "paired": stl.build_paired,
    "locus_runs": stl.build_locus_runs,
}


def _oracle_table(case):
    ot = orc.OracleTable(case.chrom_size, case.rep_len, case.n_fam, case.n_cla)
    r = case.rows
    st = ot.add_rows(r["chrom"], r["start"], r["end"], r["cons_start"], r["cons_end"], r["rep"], r["fam"], r["cla"])
    assert (st == np.arange(len(st))).all()
    return ot


def _check_hits_against_oracle(case, m):
    """Every unpaired mapped record on a chromosome of the size file: binKeeperFind on the reference's start / end gives the
    model's hits in the model's order, and nothing for a record the model says does not go on."""
    ot = _oracle_table(case)
    flag = case.rd["flag"]
    checked = 0
    for i in range(case.n):
        if m.chrom[i] < 0 or (flag[i] & 5):
            assert not m.q[i]
            continue
        got = ot.find(int(m.chrom[i]), int(m.ust[i]), int(m.uen[i]))
        want = m.hit_orig[m.hit_ptr[i]:m.hit_ptr[i + 1]]
        assert np.array_equal(got, want), (case.name, i, got, want)
        assert m.q[i] or len(got) == 0
        checked += 1
    ot.close()
    return checked


@pytest.mark.parametrize("name", sorted(BUILDERS))
def test_builder_classes_and_hits(name):
    case = BUILDERS[name]()
    assert case.n <= 20_000
    m = stl.model(case, 1 << 16)
    stl.check_promises(case, 1 << 16, m)
    assert _check_hits_against_oracle(case, m) > case.n // 4
    # the window entries of hits in LDS tiles are 1 .. wn
    lds = np.isin(m.rec_route[m.rec_of_hit], (stl.R_NARROW, stl.R_WIDE))
    assert (m.hit_entry[lds] >= 1).all() and (m.hit_entry[lds] <= m.wn[m.tile_of[m.rec_of_hit]][lds]).all()
    assert m.wn[np.isin(m.route, (stl.R_NARROW, stl.R_WIDE))].max() <= stl.WIN


def test_builders_cover_every_route_and_b():
    """In the wide tiles b runs to nb - 1, past 64 on either side; the b of a record never leaves its slice."""
    case = stl.build_slice_width()
    m = stl.model(case, 1 << 16)
    wide = m.q & (m.rec_route == stl.R_WIDE)
    assert (m.b[wide] >= 1).all() and (m.b[wide] <= m.nb[m.tile_of][wide] - 1).all() and m.b[wide].max() == 127
    narrow = m.q & (m.rec_route == stl.R_NARROW)
    assert m.b[narrow].max() == 63


@pytest.mark.parametrize("tail", [1, 255, 256, 257, 1023])
@pytest.mark.parametrize("cap", [1024, 1025, 7001])
def test_tails_and_cuts(tail, cap):
    case = stl.build_tails(8 * 1024 + tail)
    m = stl.model(case, cap)
    K = stl.classes(case, cap, m)
    assert K["n_mod_1024"] == tail
    assert K["ragged_tiles"] >= (1 if tail % 256 or cap % 256 else 0)
    # a capacity off the tile puts batch ends inside tiles; every batch starts a tile of its own
    assert (K["batch_end_inside_tile"] > 0) == (cap % 256 != 0)
    assert np.isin(np.arange(0, case.n, cap), m.t0).all()
    assert int((m.t1 - m.t0).sum()) == case.n


def test_tails_hits_against_oracle():
    case = stl.build_tails(8 * 1024 + 257)
    m = stl.model(case, 7001)
    assert _check_hits_against_oracle(case, m) > 8000


def test_spill_geometry():
    """6-bit fields take 15 tiles of 4 records a lane: 31 tiles per wave are two spills and a remainder."""
    n = stl.SPILL_N
    assert stl.tiles_per_wave(n, 3) >= 31 and stl.tiles_per_wave(n, 1) >= 93
    assert stl.tiles_per_wave(16000 * 1024, 1) == 16000 and stl.tiles_per_wave(16000 * 1024 + 1, 1) == 16001
    assert stl.tiles_per_wave(1, 8) == 1 and stl.tiles_per_wave(1025, 1) == 2
