"""A plain restatement (numpy, no device, no code shared with csrc/itx_bigwig.hip, csrc/itx_bwfold.h or host/bw_sum.c) of what a bigWig
of `iteres stat` holds for a coverage vector: the data sections, every zoom level's summaries and the zoom blocks.

The summaries follow bbiAddToSummary (cuskent/bbiWrite.c:370-421) for items that tile a sequence from 0: a summary of
reduction r over a sequence of `size` bases covers [j * r, min(j * r + r, size)); it is opened by its first item (min
and max taken from it, the count and the two sums at zero) and then takes its items ONE AFTER THE OTHER, every step
computed in float64 and stored as float32 (the fields of struct bbiSummary are floats), valid_count through
(uint32)(double). Level 0 takes the bases (count 1, min = max = sum = v, squares v * v), level k the summaries of level
k - 1. The code below is vectorised ACROSS summaries and loops over the items of a summary, so the order of the
roundings inside a summary is the sequential one."""
from __future__ import annotations

import numpy as np

ITEMS = 1024            # bases per section, summaries per zoom block
SUMMARY = np.dtype([("chrom_id", "<u4"), ("start", "<u4"), ("end", "<u4"), ("valid_count", "<u4"),
                    ("min_val", "<f4"), ("max_val", "<f4"), ("sum_data", "<f4"), ("sum_squares", "<f4")])
assert SUMMARY.itemsize == 32


def base_values(cov):
    """what a section stores for a base: (float)(double)count"""
    return np.asarray(cov, np.uint32).astype(np.float64).astype(np.float32)


def sections(cov, seqs):
    """[payload bytes] of every section in file order; seqs: (offset, length) in bigWig id order"""
    out = []
    for cid, (off, ln) in enumerate(seqs):
        vals = base_values(cov[off:off + ln])
        for s in range(0, ln, ITEMS):
            v = vals[s:s + ITEMS]
            hdr = np.array([cid, s, s + len(v), 1, 1, 3 | len(v) << 16], "<u4")          # fixedStep, step 1, span 1
            out.append(hdr.tobytes() + v.astype("<f4").tobytes())
    return out


def _fold(n_out, first_item, n_items, q, cnt, mn, mx, sd, sq):
    """n_out summaries; summary j takes items first_item[j] .. first_item[j] + n_items[j] (n_items <= q) of the item
    arrays cnt (uint32), mn, mx, sd (float32) and sq (float32; float64 for the squares of bases), in order."""
    o_vc = np.zeros(n_out, np.uint32)
    o_mn = mn[first_item].copy()
    o_mx = mx[first_item].copy()
    o_sd = np.zeros(n_out, np.float32)
    o_sq = np.zeros(n_out, np.float32)
    for t in range(q):
        live = np.nonzero(n_items > t)[0]
        if not len(live):
            break
        i = first_item[live] + t
        o_vc[live] = (o_vc[live].astype(np.float64) + cnt[i].astype(np.float64)).astype(np.uint32)
        a, b = o_mn[live], mn[i]
        o_mn[live] = np.where(a.astype(np.float64) > b.astype(np.float64), b, a)
        a, b = o_mx[live], mx[i]
        o_mx[live] = np.where(a.astype(np.float64) < b.astype(np.float64), b, a)
        o_sd[live] = (o_sd[live].astype(np.float64) + sd[i].astype(np.float64)).astype(np.float32)
        o_sq[live] = (o_sq[live].astype(np.float64) + sq[i].astype(np.float64)).astype(np.float32)
    return o_vc, o_mn, o_mx, o_sd, o_sq


def _tiles(lengths, r):
    """the summaries of reduction r over sequences of these lengths: (sequence, index inside it) per summary, and the
    first summary of every sequence"""
    per = (np.asarray(lengths, np.int64) + r - 1) // r
    first = np.concatenate([[0], np.cumsum(per)]).astype(np.int64)
    seq = np.repeat(np.arange(len(per), dtype=np.int64), per)
    j = np.arange(first[-1], dtype=np.int64) - first[seq]
    return seq, j, first


def summaries(cov, seqs, reductions):
    """[SUMMARY array] per level"""
    cov = np.asarray(cov, np.uint32)
    lengths = np.array([ln for _, ln in seqs], np.int64)
    out = []
    prev_first = None
    for k, r in enumerate(reductions):
        r = int(r)
        seq, j, first = _tiles(lengths, r)
        n = len(seq)
        rec = np.zeros(n, SUMMARY)
        if n:
            start = j * r
            end = np.minimum(start + r, lengths[seq])
            rec["chrom_id"], rec["start"], rec["end"] = seq, start, end
            if k == 0:
                # the items are the bases: one float each, squares formed in float64
                vals = np.concatenate([base_values(cov[o:o + ln]) for o, ln in seqs])
                vbase = np.concatenate([[0], np.cumsum(lengths)])[:-1]
                sqv = vals.astype(np.float64) * vals.astype(np.float64)
                # the square stays float64 until it is added (_fold converts its items to float64 itself)
                o_vc, o_mn, o_mx, o_sd, o_sq = _fold(n, vbase[seq] + start, end - start, r, np.ones(len(vals), np.uint32),
                                                     vals, vals, vals, sqv)
            else:
                q, rem = divmod(r, int(reductions[k - 1]))
                assert rem == 0 and q >= 1, "a level takes whole summaries of the one before"
                p = out[-1]
                fi = prev_first[seq] + j * q
                cnt_items = np.minimum(fi + q, prev_first[seq + 1]) - fi
                o_vc, o_mn, o_mx, o_sd, o_sq = _fold(n, fi, cnt_items, q, p["valid_count"], p["min_val"], p["max_val"],
                                                     p["sum_data"], p["sum_squares"])
            rec["valid_count"], rec["min_val"], rec["max_val"], rec["sum_data"], rec["sum_squares"] = o_vc, o_mn, o_mx, o_sd, o_sq
        out.append(rec)
        prev_first = first
    return out


def zoom_blocks(level):
    """[payload bytes] of one level's zoom blocks: 1024 summaries each, the last one shorter"""
    raw = level.tobytes()
    return [raw[i:i + 32 * ITEMS] for i in range(0, len(raw), 32 * ITEMS)]


def build(cov, seqs, reductions):
    """{"sections": [bytes], "levels": [SUMMARY array], "zoom": [[bytes] per level]}"""
    lv = summaries(cov, seqs, reductions)
    return {"sections": sections(cov, seqs), "levels": lv, "zoom": [zoom_blocks(x) for x in lv]}
