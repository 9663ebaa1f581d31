"""A model of k_stream's tiles, and inputs built to land on every threshold of its routes. Plain numpy: no GPU, no engine.

k_stream (iteres_amd/csrc/itx_stream.hip) decides per 256-record tile how it looks its records up: record by record
from global memory, through an LDS window with a narrow (<= 64 bins) or wide (<= 128 bins) slice of the binned index,
or per lane from global memory when the tile spans more than 128 bins or more than ITX_WIN = 128 rows. This module
restates that geometry from the kernel's documentation (it never calls the kernel) so that a test can say, before it
runs the engine, how many tiles and records of its input sit on each side of every comparison. test_stream_tiles_model
proves the model's hit lists against the oracle's binKeeperFind; test_gpu_stream_paths runs the engine on the inputs.

Tiles. A launch gives every workgroup a span of records that is a multiple of ITX_STREAM_TILE = 1024 (itx_stream_plan),
and wave w of a workgroup takes the 256 records from begin + 256 w + 1024 k. So the tiles of a submitted batch are its
aligned groups of 256 consecutive records, whatever the number of workgroups; the engine cuts the stream into batches
at batch_capacity. The partition path was checked for the same alignment: itx_part_run (itx_partition.hip) takes its
span from the same itx_stream_plan and hands it to itx_launch_stream, which refuses any span that is not a multiple of
the tile; only the number of workgroups may be capped there (max_blocks), which moves no tile.

Index (itx_tablebuild.h). The rows of a chromosome are sorted stably by start; bl[g].x is the number of rows with
s < g << shift, bl[g].y the first row whose prefix-maximum end exceeds g << shift. The builders keep the genome below
about 8 Mbp with a few thousand rows, so shift is 7; the GPU test asserts TableInfo.bin_shift == SHIFT.

List order (binKeeperFind, binRange.c:196-227): UCSC levels coarse to fine, bins descending, file order ascending.

The model covers single-end records with extension = 0. Paired records are known to it only by their flag (builder 5).
"""
from __future__ import annotations

import numpy as np

SHIFT = 7
TILE = 256                    # records per wave and tile
WG_TILE = 1024                # ITX_STREAM_TILE: four waves
WIN = 128                     # ITX_WIN
R_NONE, R_RECORD, R_NARROW, R_WIDE, R_GLOBAL = 0, 1, 2, 3, 4
SPILL_N = 3 * 31 * WG_TILE + 257     # at three workgroups every wave still walks 31 tiles: two spills of the 6-bit fields and a rest


class Case:
    """One input: table rows (dict of arrays, file order), sizes, the header's tid -> chromosome map and the records."""

    def __init__(self, name, rows, chrom_size, rep_len, n_fam, n_cla, tid2chrom, rd):
        self.name = name
        self.rows = {k: np.asarray(v, np.int64) for k, v in rows.items()}
        self.chrom_size = np.asarray(chrom_size, np.int64)
        self.rep_len = np.asarray(rep_len, np.uint32)
        self.n_fam, self.n_cla = int(n_fam), int(n_cla)
        self.tid2chrom = np.asarray(tid2chrom, np.int32)
        self.rd = rd
        self.n = len(rd["tid"])
        assert int(self.chrom_size.sum()) <= 8_200_000 and len(self.rows["chrom"]) < 40_000      # shift stays 7


def _mk_rows(chrom, start, end, rng, rep_len):
    n = len(start)
    rep = rng.integers(0, len(rep_len), n)
    return {"chrom": np.asarray(chrom, np.int64), "start": np.asarray(start, np.int64), "end": np.asarray(end, np.int64),
            "cons_start": rng.integers(0, 60, n), "cons_end": rng.integers(10, 1500, n), "rep": rep, "fam": rep % 3, "cla": rep % 2}


def _mk_reads(tid, pos, tmpend, rng, flag=None, mapq=None):
    n = len(pos)
    return {"tid": np.asarray(tid, np.int32) if np.ndim(tid) else np.full(n, tid, np.int32),
            "pos": np.asarray(pos, np.int64).astype(np.int32), "tmpend": np.asarray(tmpend, np.int64).astype(np.int32),
            "mapq": rng.integers(0, 61, n).astype(np.uint8) if mapq is None else np.asarray(mapq, np.uint8),
            "flag": np.where(rng.random(n) < 0.5, 16, 0).astype(np.uint16) if flag is None else np.asarray(flag, np.uint16),
            "mpos": np.zeros(n, np.int32), "isize": np.zeros(n, np.int32)}


def _cat_reads(parts):
    return {k: np.concatenate([p[k] for p in parts]) for k in parts[0]}


REP_LEN = np.array([400, 0, 50, 1000], np.uint32)          # a zero-length consensus among them; cons_end runs to 1500


# ---------------------------------------------------------------------------------------------------------------- index
def _ucsc_level_bin(s, e):
    sb, eb = s >> 17, (e - 1) >> 17
    lvl = np.full(len(s), -1, np.int64)
    b = np.zeros(len(s), np.int64)
    for i in range(6):
        hit = (lvl < 0) & (sb == eb)
        lvl[hit] = i
        b[hit] = sb[hit]
        sb, eb = sb >> 3, eb >> 3
    assert (lvl >= 0).all()
    return lvl, b


class ChromIndex:
    def __init__(self, file_ids, s, e, size):
        o = np.argsort(s, kind="stable")
        self.orig = file_ids[o]                                  # sorted position -> file row
        self.s, self.e = s[o], e[o]
        self.pmax = np.maximum.accumulate(self.e) if len(o) else self.e
        bound = np.arange((int(size) >> SHIFT) + 2, dtype=np.int64) << SHIFT
        self.x = np.searchsorted(self.s, bound, "left")          # rows with s < bound
        self.y = np.searchsorted(self.pmax, bound, "right")      # first row whose prefix-max end > bound
        lvl, b = _ucsc_level_bin(self.s, self.e) if len(o) else (self.s, self.s)
        lo = np.lexsort((self.orig, -b, -lvl))                   # level coarse -> fine, bin descending, file order
        self.rank = np.empty(len(o), np.int64)
        self.rank[lo] = np.arange(len(o))


def build_index(case):
    r = case.rows
    out = []
    for c, size in enumerate(case.chrom_size):
        ids = np.flatnonzero(r["chrom"] == c)
        out.append(ChromIndex(ids, r["start"][ids], r["end"][ids], size))
    return out


# ---------------------------------------------------------------------------------------------------------------- model
def _i32(u):
    return (np.asarray(u, np.int64) & 0xFFFFFFFF).astype(np.uint32).view(np.int32).astype(np.int64)


class Model:
    """Per record: chrom, q (goes on to the lookup), odd, qs, qe, ust/uen (the reference's start / end as signed ints: what
    binKeeperFind is called with), b, hits (CSR: hit_ptr, hit_sorted, hit_orig, hit_rank, hit_ov, in list order).
    Per tile: t0, t1, full, uniform, odd, anyq, tchrom, bin_lo, nb, lo_w, wn, route."""


def model(case, batch_capacity):
    m = Model()
    idx = build_index(case)
    m.index = idx
    rd, n = case.rd, case.n
    tid = rd["tid"].astype(np.int64)
    ntid = len(case.tid2chrom)
    in_hdr = (tid >= 0) & (tid < ntid)
    chrom = np.where(in_hdr, case.tid2chrom[np.clip(tid, 0, ntid - 1)], -1).astype(np.int64)
    size = np.where(chrom >= 0, case.chrom_size[np.clip(chrom, 0, None)], 0)
    cend = (size - 1) & 0xFFFFFFFF
    flag = rd["flag"].astype(np.int64)
    paired = (flag & 1) != 0
    ust = rd["pos"].astype(np.int64) & 0xFFFFFFFF
    uen = np.minimum(cend, rd["tmpend"].astype(np.int64) & 0xFFFFFFFF)
    sti, eni = _i32(ust), _i32(uen)
    qs, qe = np.maximum(sti, 0), np.minimum(eni, size)
    has_rows = np.array([len(ix.s) > 0 for ix in idx] + [False])[chrom]        # chrom -1 -> the appended False
    q = ((flag & 4) == 0) & (chrom >= 0) & (cend != 1) & (qs < qe) & has_rows & ~paired
    m.chrom, m.q, m.qs, m.qe, m.ust, m.uen, m.paired = chrom, q, qs, qe, sti, eni, paired
    m.odd_rec = q & ((sti != qs) | (eni != qe))
    # hits of every record that goes on, in list order
    ptr = np.zeros(n + 1, np.int64)
    hs, ho, hr, hv = [], [], [], []
    for c, ix in enumerate(idx):
        recs = np.flatnonzero(q & (chrom == c))
        for a in range(0, len(recs), 2048):
            rr = recs[a:a + 2048]
            ov = np.minimum(ix.e[None, :], qe[rr, None]) - np.maximum(ix.s[None, :], qs[rr, None])
            ri, ci = np.nonzero(ov > 0)
            o = np.lexsort((ix.rank[ci], ri))
            ri, ci = ri[o], ci[o]
            np.add.at(ptr, rr[ri] + 1, 1)
            hs.append((rr[ri], ci, ix.orig[ci], ix.rank[ci], ov[ri, ci]))
    if hs:
        rec = np.concatenate([h[0] for h in hs])
        o = np.argsort(rec, kind="stable")
        m.hit_sorted, m.hit_orig, m.hit_rank, m.hit_ov = (np.concatenate([h[k] for h in hs])[o] for k in (1, 2, 3, 4))
    else:
        m.hit_sorted = m.hit_orig = m.hit_rank = m.hit_ov = np.zeros(0, np.int64)
    m.hit_ptr = np.cumsum(ptr)
    m.nhits = np.diff(m.hit_ptr)
    # tiles
    T = {k: [] for k in ("t0", "t1", "full", "uniform", "odd", "anyq", "tchrom", "bin_lo", "nb", "lo_w", "wn", "route", "batch")}
    m.b = np.zeros(n, np.int64)
    m.tile_of = np.zeros(n, np.int64)
    for bi, b0 in enumerate(range(0, n, batch_capacity)):
        b1 = min(b0 + batch_capacity, n)
        for t0 in range(b0, b1, TILE):
            t1 = min(t0 + TILE, b1)
            sl = slice(t0, t1)
            m.tile_of[sl] = len(T["t0"])
            uniform = bool((tid[sl] == tid[t0]).all())
            tq = q[sl] if uniform else np.zeros(t1 - t0, bool)
            odd = (not uniform) or bool(m.odd_rec[sl].any())
            anyq = bool(tq.any())
            c = int(chrom[t0]) if uniform else -1
            bin_lo = nb = lo_w = wn = -1
            if odd:
                route = R_RECORD
            elif not anyq:
                route = R_NONE
            else:
                mn, mx = int(qs[sl][tq].min()), int(qe[sl][tq].max())
                bin_lo = mn >> SHIFT
                nb = (mx >> SHIFT) + 1 - bin_lo + 1
                ix = idx[c]
                lo_w = int(ix.y[bin_lo])
                wn = max(int(ix.x[(mx >> SHIFT) + 1]) - lo_w, 0)
                route = R_GLOBAL if nb > 128 or wn > WIN else (R_WIDE if nb > 64 else R_NARROW)
                m.b[sl] = np.where(tq, (qe[sl] >> SHIFT) - bin_lo + 1, 0)
            for k, v in (("t0", t0), ("t1", t1), ("full", t1 - t0 == TILE), ("uniform", uniform), ("odd", odd), ("anyq", anyq),
                         ("tchrom", c), ("bin_lo", bin_lo), ("nb", nb), ("lo_w", lo_w), ("wn", wn), ("route", route), ("batch", bi)):
                T[k].append(v)
    for k, v in T.items():
        setattr(m, k, np.array(v))
    m.n_tiles = len(m.t0)
    m.rec_route = m.route[m.tile_of]
    # window entry of every hit (meaningful in LDS tiles): sorted row - lo_w + 1
    rec_of_hit = np.repeat(np.arange(n), m.nhits)
    m.rec_of_hit = rec_of_hit
    m.hit_entry = m.hit_sorted - m.lo_w[m.tile_of[rec_of_hit]] + 1
    return m


def tiles_per_wave(n, blocks):
    """The most tiles any wave walks in one launch of n records over `blocks` workgroups (itx_stream_plan)."""
    sp = -(-n // blocks)
    sp = max(-(-sp // WG_TILE) * WG_TILE, WG_TILE)
    end = min(sp, n)                                               # workgroup 0 has the fullest span
    return -(-end // WG_TILE)                                      # wave 0: tiles at 0, 1024, ...


def classes(case, batch_capacity, m=None):
    """Counts of tiles / records in every named class."""
    m = m or model(case, batch_capacity)
    K = {}
    lds = (m.route == R_NARROW) | (m.route == R_WIDE)
    reached = (m.route >= R_NARROW)                                # the tile got as far as nb / wn
    for v in (2, 3, 5, 63, 64, 65, 66, 127, 128, 129, 130):
        K[f"nb{v}"] = int((reached & (m.nb == v) & (m.wn <= 64)).sum())
    rl = m.q & (m.rec_route >= R_NARROW)
    wide_rec = m.q & (m.rec_route == R_WIDE)
    for v in (1, 63, 64, 65, 126, 127):
        K[f"wide_b{v}"] = int((wide_rec & (m.b == v)).sum())
        K[f"wide_b{v}_hit"] = int((wide_rec & (m.b == v) & (m.nhits >= 1)).sum())      # ... that a wrong top would lose
    for v in (0, 1, 127, 128, 129, 130):
        K[f"wn{v}_narrow"] = int((reached & (m.nb <= 64) & (m.wn == v)).sum())
    for v in (128, 129):
        K[f"wn{v}_wide"] = int((reached & (m.nb >= 65) & (m.nb <= 128) & (m.wn == v)).sum())
    in_lds = m.q & ((m.rec_route == R_NARROW) | (m.rec_route == R_WIDE))
    one = in_lds & (m.nhits == 1) & (m.wn[m.tile_of] == 128)
    first_entry = np.zeros(case.n, np.int64)
    hp = m.hit_ptr[:-1]
    ok = m.nhits > 0
    first_entry[ok] = m.hit_entry[hp[ok]]
    K["wn128_only_entry1"] = int((one & (first_entry == 1)).sum())
    K["wn128_only_entry128"] = int((one & (first_entry == 128)).sum())
    for k in range(7):
        K[f"hits{k}"] = int((in_lds & (m.nhits == k)).sum())
    K["hits8plus"] = int((in_lds & (m.nhits >= 8)).sum())
    two = np.flatnonzero(in_lds & (m.nhits == 2))
    a, b = m.hit_ptr[two], m.hit_ptr[two] + 1                      # first / second in list order
    eq = m.hit_ov[a] == m.hit_ov[b]
    low_first = m.hit_sorted[a] < m.hit_sorted[b]
    K["two_eq_lowfirst"] = int((eq & low_first).sum())
    K["two_eq_lowsecond"] = int((eq & ~low_first).sum())
    K["two_first_more"] = int((m.hit_ov[a] > m.hit_ov[b]).sum())
    K["two_first_less"] = int((m.hit_ov[a] < m.hit_ov[b]).sum())
    # list order that differs from start order among the hits of one record
    if len(m.hit_sorted) > 1:
        same = m.rec_of_hit[1:] == m.rec_of_hit[:-1]
        K["list_order_not_start_order"] = int(np.unique(m.rec_of_hit[1:][same & (m.hit_sorted[1:] < m.hit_sorted[:-1])]).size)
    else:
        K["list_order_not_start_order"] = 0
    hit_in_lds = in_lds[m.rec_of_hit]
    rlen = case.rep_len[case.rows["rep"][m.hit_orig]].astype(np.int64)
    K["hit_cons_end_past"] = int((hit_in_lds & (case.rows["cons_end"][m.hit_orig] > rlen)).sum())
    K["hit_zero_len"] = int((hit_in_lds & (rlen == 0)).sum())
    # routes
    for name, r in (("none", R_NONE), ("record", R_RECORD), ("narrow", R_NARROW), ("wide", R_WIDE), ("global", R_GLOBAL)):
        K[f"route_{name}"] = int((m.route == r).sum())
    tid = case.rd["tid"].astype(np.int64)
    ntid = len(case.tid2chrom)
    for at in (1, 128, 255):
        K[f"refchange_at{at}"] = 0
    K["tile_bad_tids"] = K["tile_one_negpos"] = K["tile_norows"] = K["tile_no_q"] = 0
    for t in range(m.n_tiles):
        sl = slice(m.t0[t], m.t1[t])
        ch = np.flatnonzero(tid[sl][1:] != tid[sl][:-1]) + 1
        if m.full[t] and len(ch) == 1 and int(ch[0]) in (1, 128, 255):
            K[f"refchange_at{int(ch[0])}"] += 1
        K["tile_bad_tids"] += int((tid[sl] >= ntid).any() and (tid[sl] == -1).any())
        K["tile_one_negpos"] += int((m.odd_rec[sl] & (case.rd["pos"][sl] < 0)).sum() == 1)
        c = m.tchrom[t]
        K["tile_norows"] += int(m.uniform[t] and c >= 0 and len(m.index[c].s) == 0)
        K["tile_no_q"] += int(m.uniform[t] and c >= 0 and len(m.index[c].s) > 0 and not m.anyq[t])
    size = np.where(m.chrom >= 0, case.chrom_size[np.clip(m.chrom, 0, None)], 0)
    K["rec_past_end"] = int((m.q & (case.rd["tmpend"].astype(np.int64) > size)).sum())
    K["rec_past_end_lds"] = int((in_lds & (case.rd["tmpend"].astype(np.int64) > size)).sum())
    # paired batches
    K["have_pe"] = int(m.paired.any())
    K["pairfree_then_lastpaired"] = K["tile_all_paired"] = 0
    for t in range(m.n_tiles):
        p = m.paired[m.t0[t]:m.t1[t]]
        K["tile_all_paired"] += int(m.full[t] and p.all())
        if t + 1 < m.n_tiles and m.batch[t] == m.batch[t + 1] and m.full[t] and m.full[t + 1] and not p.any():
            p2 = m.paired[m.t0[t + 1]:m.t1[t + 1]]
            K["pairfree_then_lastpaired"] += int(p2[-1] and not p2[:-1].any())
    # tails
    K["n_mod_1024"] = case.n % WG_TILE
    K["ragged_tiles"] = int((~m.full).sum())
    K["batch_end_inside_tile"] = int(((m.t1 - m.t0 != TILE) & (m.t1 != case.n)).sum())
    # locus runs: the row a record with at most one hit chooses (-1: none), as lanes x 4
    K["locus_full_tiles"] = K["locus_broken"] = K["locus_alt_record"] = K["locus_alt_lane"] = K["locus_end63"] = K["locus_start0"] = 0
    chosen = np.full(case.n, -1, np.int64)
    chosen[ok] = m.hit_orig[hp[ok]]
    chosen[m.nhits > 1] = -2                                       # not decided by the model
    for t in range(m.n_tiles):
        if not m.full[t] or m.route[t] not in (R_NARROW, R_WIDE):
            continue
        v = chosen[m.t0[t]:m.t1[t]]
        if (v == -2).any():
            continue
        K["locus_full_tiles"] += int(v[0] >= 0 and (v == v[0]).all())
        K["locus_alt_record"] += int(v[0] >= 0 and v[1] >= 0 and v[0] != v[1] and (v[0::2] == v[0]).all() and (v[1::2] == v[1]).all())
        g = v.reshape(64, 4)                                       # lane, j
        K["locus_alt_lane"] += int(g[0, 0] >= 0 and g[1, 0] >= 0 and g[0, 0] != g[1, 0] and (g[0::2] == g[0, 0]).all() and (g[1::2] == g[1, 0]).all())
        for j in range(4):
            s = g[:, j]
            K["locus_broken"] += int(((s[1:-1] < 0) & (s[:-2] >= 0) & (s[:-2] == s[2:])).sum())
            K["locus_end63"] += int(s[63] >= 0 and s[62] == s[63] and (s != s[63]).any())
            K["locus_start0"] += int(s[0] >= 0 and s[1] == s[0] and (s != s[0]).any())
    return K


# ------------------------------------------------------------------------------------------------------------- builders
NB_SET = (2, 3, 5, 63, 64, 65, 66, 127, 128, 129, 130)
B_SET = (1, 63, 64, 65, 126, 127)


def _binned_tile(A, nb, rng, special=()):
    """256 sorted reads of 20 bp, each inside one bin, spanning exactly nb - 1 bins from A (a multiple of 128): nb as the kernel
    counts it. `special`: values of b that get at least four reads. Returns (pos, b)."""
    top = nb - 1
    b = [1, top] + [v for v in special if v <= top for _ in range(4)]
    b = np.array(b + list(rng.integers(1, top + 1, TILE - len(b))))
    pos = A + (b - 1) * 128 + rng.integers(0, 100, TILE)
    o = np.argsort(pos, kind="stable")
    return pos[o], b[o]


def build_slice_width(seed=101):
    """Builder 1: two tiles for every nb in NB_SET, each with at most 64 rows under it; the wide ones hold reads at b in B_SET,
    every one of them over a row, so a top taken from the wrong half of the slice loses or invents a hit."""
    rng = np.random.default_rng(seed)
    cur = 128 * 40
    rs, re, parts = [], [], []
    for nb in NB_SET:
        for _ in range(2):
            pos, b = _binned_tile(cur, nb, rng, B_SET if nb > 64 else ())
            want = sorted({1, nb - 1} | {v for v in B_SET if v <= nb - 1 and nb > 64})
            rest = np.setdiff1d(np.unique(b), want)
            extra = rng.choice(rest, min(len(rest), 40 - len(want)), replace=False) if len(rest) else []
            for v in sorted(set(want) | set(int(x) for x in extra)):
                rs.append(cur + (v - 1) * 128 + 5)
                re.append(cur + (v - 1) * 128 + 123)
            parts.append(_mk_reads(0, pos, pos + 20, rng))
            cur += nb * 128 + 1024
    size = 1_000_000
    assert cur < size
    p = rng.permutation(len(rs))
    rows = _mk_rows(np.zeros(len(rs)), np.array(rs)[p], np.array(re)[p], rng, REP_LEN)
    return Case("slice_width", rows, [size], REP_LEN, 3, 2, [0], _cat_reads(parts))


WN_SET = ((0, 20), (1, 20), (127, 20), (128, 20), (129, 20), (130, 20), (128, 100), (129, 100))


def build_window_size(seed=102):
    """Builder 2: tiles with exactly wn disjoint rows under them, two for every (wn, nb) of WN_SET. Reads of 8 bp sit inside one
    row (one hit: the window entry of row i is i + 1) or in a gap; every tile has reads on its first and on its last row."""
    rng = np.random.default_rng(seed)
    cur = 128 * 40
    rs, re, parts = [], [], []
    for wn, nb in WN_SET:
        for _ in range(2):
            nbins = nb - 1
            sp = (nbins * 128 - 16) // max(wn, 1)
            s = cur + 8 + sp * np.arange(wn)
            e = s + (min(sp, 100) - 3)
            rs += list(s)
            re += list(e)
            pos = [cur, cur + nbins * 128 - 20]                          # anchors: first and last bin
            if wn:
                on = np.concatenate([np.zeros(8, np.int64), np.full(8, wn - 1), rng.integers(0, wn, 200)])
                pos += list(s[on] + 2)
                gap = rng.integers(0, wn, TILE - len(pos))
                pos += list(e[gap])                                      # [e, e + 2): between two rows
                ln = np.array([8, 8] + [8] * len(on) + [2] * len(gap))
            else:
                pos += list(cur + rng.integers(0, nbins * 128 - 20, TILE - 2))
                ln = np.full(TILE, 8)
            pos = np.array(pos)
            o = np.argsort(pos, kind="stable")
            parts.append(_mk_reads(0, pos[o], (pos + ln)[o], rng))
            cur += nb * 128 + 1024
    size = 1_000_000
    assert cur < size
    p = rng.permutation(len(rs))
    rows = _mk_rows(np.zeros(len(rs)), np.array(rs)[p], np.array(re)[p], rng, REP_LEN)
    return Case("window_size", rows, [size], REP_LEN, 3, 2, [0], _cat_reads(parts))


def build_hit_counts(seed=103):
    """Builder 3: nested stacks of nine rows (reads beside the centre overlap 0 .. 9 of them) and pairs of staggered rows (two
    hits with equal or unequal overlaps). Some stacks sit on a 128 kb and on a 1 Mb boundary of the UCSC bin scheme, so
    their outer rows are on coarser levels and come first in list order; the file order is shuffled, so list order inside
    a bin differs from start order too."""
    rng = np.random.default_rng(seed)
    size = 2_200_000
    starts = sorted([5000, 131072 - 330, 262144 - 730, 400_000, 5 * 131072 - 330, 1048576 - 330, 1048576 + 5000, 2_000_000])
    rs, re, parts = [], [], []
    for A in starts:
        pos, end = [], []
        for c in (A + 300, A + 700):
            i = np.arange(9)
            rs += list(c - 10 * i - 5)
            re += list(c + 10 * i + 5)
            for _ in range(3):
                pos.append(c - 3); end.append(c + 3)                     # nine hits
                for j in range(9):
                    pos.append(c + 5 + 10 * j); end.append(c + 9 + 10 * j)          # 8 - j hits
                    pos.append(c - 9 - 10 * j); end.append(c - 5 - 10 * j)
        for k in range(10):
            p = A + 1000 + 150 * k
            rs += [p, p + 20]
            re += [p + 40, p + 60]
            for _ in range(3):
                for a, b in ((p + 10, p + 30), (p + 30, p + 50), (p + 20, p + 40), (p + 22, p + 38)):
                    pos.append(a); end.append(b)
        extra = TILE - len(pos)
        q = A + rng.integers(0, 2600, extra)
        pos += list(q)
        end += list(q + rng.integers(1, 120, extra))
        pos, end = np.array(pos), np.array(end)
        o = np.argsort(pos, kind="stable")
        parts.append(_mk_reads(0, pos[o], end[o], rng))
    p = rng.permutation(len(rs))
    rows = _mk_rows(np.zeros(len(rs)), np.array(rs)[p], np.array(re)[p], rng, REP_LEN)
    return Case("hit_counts", rows, [size], REP_LEN, 3, 2, [0], _cat_reads(parts))


def _random_rows(rng, chrom, size, n, edges=False):
    s = rng.integers(200, size - 1000, n)
    if edges:                                                             # near the two ends, where builder 4 reads
        s = np.where(rng.random(n) < 0.5, s % 30_000 + 200, size - 31_000 + s % 30_000)
    s = np.sort(s)
    e = s + rng.integers(50, 300, n)
    s = np.concatenate([[0], s, [size - 200]])
    e = np.concatenate([[100], e, [size]])
    return np.full(len(s), chrom), s, e


def _sorted_reads(rng, tid, lo, hi, n, **kw):
    pos = np.sort(rng.integers(lo, hi, n))
    return _mk_reads(tid, pos, pos + rng.integers(30, 60, n), rng, **kw)


def build_record_route(seed=104):
    """Builder 4: tiles the kernel takes record by record, and tiles without a lookup. Header: tid 0, 1 have rows, tid 2 is a
    chromosome without rows, tid 3 is not in the size file. The tiles are sorted inside, not against each other."""
    rng = np.random.default_rng(seed)
    sizes = [400_000, 300_000, 100_000]
    c0, s0, e0 = _random_rows(rng, 0, sizes[0], 300, edges=True)
    c1, s1, e1 = _random_rows(rng, 1, sizes[1], 300, edges=True)
    c, s, e = np.concatenate([c0, c1]), np.concatenate([s0, s1]), np.concatenate([e0, e1])
    p = rng.permutation(len(s))
    rows = _mk_rows(c[p], s[p], e[p], rng, REP_LEN)
    parts = []
    for k in (1, 128, 255):                                               # the reference changes at record k
        a = _sorted_reads(rng, 0, sizes[0] - 30_000, sizes[0] - 20, k)
        a["tmpend"][-1] = sizes[0] + 7                                    # ... and the last one reaches past the end
        parts += [a, _sorted_reads(rng, 1, 0, 30_000, TILE - k)]
    t = _sorted_reads(rng, 0, 0, 30_000, TILE)
    t["tid"][17], t["tid"][200] = 9, -1                                   # beyond the header, and no reference
    parts.append(t)
    t = _sorted_reads(rng, 0, 0, 30_000, TILE)
    t["pos"][0], t["tmpend"][0] = -5, 35                                  # unsigned start != clipped query start
    parts.append(t)
    parts.append(_sorted_reads(rng, 2, 0, 90_000, TILE))                  # a chromosome without rows
    parts.append(_sorted_reads(rng, 0, 100_000, 130_000, TILE, flag=np.full(TILE, 4)))      # nobody goes on
    t = _sorted_reads(rng, 0, sizes[0] - 3000, sizes[0] - 10, TILE)       # uniform, on the last rows, over the end
    t["tmpend"][-6:] = sizes[0] + np.arange(6)
    parts.append(t)
    parts.append(_sorted_reads(rng, 3, 0, 30_000, TILE))                  # not in the size file
    parts.append(_sorted_reads(rng, 1, 0, 2000, 77))                      # ragged, from position 0
    return Case("record_route", rows, sizes, REP_LEN, 3, 2, [0, 1, 2, -1], _cat_reads(parts))


def build_paired(seed=105):
    """Builder 5: a batch with mate arrays in which three tiles have no paired record and the tile after each has one: its
    last; one tile is all pairs. The mate fields of unpaired records hold values that must not be looked at."""
    rng = np.random.default_rng(seed)
    size = 500_000
    c, s, e = _random_rows(rng, 0, size, 1500)
    p = rng.permutation(len(s))
    rows = _mk_rows(c[p], s[p], e[p], rng, REP_LEN)
    parts = []
    lo = 1000

    def tile(paired_at):
        nonlocal lo
        t = _sorted_reads(rng, 0, lo, lo + 5000, TILE)
        lo += 5000
        t["mpos"][:] = rng.integers(0, size, TILE)                        # noise under unpaired records
        t["isize"][:] = rng.integers(-400, 400, TILE)
        for k in paired_at:
            kind = rng.integers(0, 6)
            fwd = rng.random() < 0.5
            isz = int(rng.integers(60, 700))                              # some beyond -I 500
            t["flag"][k] = 1 | (0 if fwd else 16) | (64 if kind else 128) | (8 if kind == 1 else 0)
            t["isize"][k] = isz if fwd else -isz
            t["mpos"][k] = t["pos"][k] + (isz - 40 if fwd else -(isz - 40))
            if kind == 2:
                t["isize"][k] = 0
        return t
    for _ in range(3):
        parts += [tile(()), tile((TILE - 1,))]
    parts += [tile(range(TILE)), tile(()), tile(range(0, TILE, 7)), tile(())]
    rd = _cat_reads(parts)
    rd["mpos"] = np.maximum(rd["mpos"], 0).astype(np.int32)
    return Case("paired", rows, [size], REP_LEN, 3, 2, [0], rd)


def build_tails(n, seed=106):
    """Builder 6: n dense sorted reads (3 % unmapped) over 500 rows: for ragged tails, batch cuts and the counters' spills."""
    rng = np.random.default_rng(seed)
    size = 1_000_000
    c, s, e = _random_rows(rng, 0, size, 500)
    p = rng.permutation(len(s))
    rows = _mk_rows(c[p], s[p], e[p], rng, REP_LEN)
    flag = np.where(rng.random(n) < 0.5, 16, 0) | np.where(rng.random(n) < 0.03, 4, 0)
    return Case(f"tails_{n}", rows, [size], REP_LEN, 3, 2, [0], _sorted_reads(rng, 0, 0, size - 100, n, flag=flag))


def build_locus_runs(seed=107):
    """Builder 7 (filter mode: one atomic per run of equal rows over the lanes of a wave, per record slot j of the lanes). Forty
    disjoint rows; lane L of a tile holds records 4 L .. 4 L + 3. The reads are placed by row, not sorted."""
    rng = np.random.default_rng(seed)
    size = 200_000
    s = 1000 + 200 * np.arange(40)
    e = s + 150
    p = rng.permutation(40)
    rows = _mk_rows(np.zeros(40), s[p], e[p], rng, REP_LEN)
    parts = []

    def tile(row_of_record, n=TILE):                                      # row -1: the gap after row 1
        r = np.asarray(row_of_record)
        pos = np.where(r >= 0, s[np.maximum(r, 0)] + rng.integers(0, 100, n), e[1] + 5)
        return _mk_reads(0, pos, pos + 30, rng, flag=np.zeros(n), mapq=np.full(n, 40))
    parts.append(tile(np.zeros(TILE, np.int64)))                         # 256 records on one row
    r = np.full((64, 4), 1)
    r[5, :] = -1; r[20, 1] = -1; r[40, 3] = -1; r[63, 0] = -1; r[0, 2] = -1; r[30:32, 0] = -1
    parts.append(tile(r.reshape(-1)))                                    # runs broken by lanes without a hit
    parts.append(tile(2 + (np.arange(TILE) & 1)))                        # two rows alternating record by record
    parts.append(tile(4 + ((np.arange(TILE) >> 2) & 1)))                 # ... and lane by lane
    lane = np.arange(TILE) >> 2
    parts.append(tile(np.where(lane < 10, 6, np.where(lane < 50, 7, 8))))      # a run from lane 0, a run up to lane 63
    parts.append(tile(lane % 40))                                        # runs of one lane
    parts.append(tile(rng.integers(-1, 40, TILE)))
    parts.append(tile(np.full(100, 9), 100))                             # ragged
    return Case("locus_runs", rows, [size], REP_LEN, 3, 2, [0], _cat_reads(parts))


# what every builder promises, as minimum counts of classes(); the tests assert these (GPU tests before they run the engine)
PROMISES = {
    "slice_width": dict({f"nb{v}": 2 for v in NB_SET}, **{f"wide_b{v}": 4 for v in B_SET}, **{f"wide_b{v}_hit": 4 for v in B_SET}, route_global=4, route_wide=8, route_narrow=10),
    "window_size": dict({f"wn{v}_narrow": 2 for v in (0, 1, 127, 128, 129, 130)}, wn128_wide=2, wn129_wide=2,
                        wn128_only_entry1=8, wn128_only_entry128=8, route_global=6),
    "hit_counts": dict({f"hits{k}": 50 for k in range(7)}, hits8plus=50, two_eq_lowfirst=20, two_eq_lowsecond=20, two_first_more=20,
                       two_first_less=20, hit_cons_end_past=100, hit_zero_len=100, list_order_not_start_order=200, route_narrow=8),
    "record_route": dict(refchange_at1=1, refchange_at128=1, refchange_at255=1, tile_bad_tids=1, tile_one_negpos=1, tile_norows=1,
                         tile_no_q=1, rec_past_end=4, rec_past_end_lds=4, route_record=5, route_none=3, ragged_tiles=1),
    "paired": dict(have_pe=1, pairfree_then_lastpaired=3, tile_all_paired=1),
    "locus_runs": dict(locus_full_tiles=1, locus_broken=6, locus_alt_record=1, locus_alt_lane=1, locus_end63=4, locus_start0=4,
                       ragged_tiles=1),
}


def check_promises(case, batch_capacity, m=None):
    K = classes(case, batch_capacity, m)
    want = PROMISES[case.name]
    short = {k: (K[k], v) for k, v in want.items() if K[k] < v}
    assert not short, f"{case.name}: classes below their promised minimum (have, want): {short}"
    return K
