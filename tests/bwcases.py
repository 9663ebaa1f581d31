"""Inputs shared by the bigWig tests: seeded coverage vectors of the content classes the writers meet (and the ones
that make their float arithmetic round), and the pile-up run whose wig is deep enough for the rounding regime."""
import os

import numpy as np

from iteres_amd import synth

CONTENT = ("small", "spikes", "plateaus", "sawtooth", "around_2p24", "uniform_u32", "near_u32_max", "pileup")


def content(kind, n, seed):
    """uint32 coverage of n bases"""
    rng = np.random.default_rng([seed, CONTENT.index(kind)])
    if kind == "small":                      # the exact regime: runs of small counts
        runs = rng.integers(1, 200, n // 50 + 2)
        v = np.repeat(np.where(rng.random(len(runs)) < 0.6, rng.integers(0, 60, len(runs)), 0), runs)
        while len(v) < n:
            v = np.concatenate([v, v])
        return v[:n].astype(np.uint32)
    if kind == "spikes":
        v = np.zeros(n, np.uint32)
        k = rng.choice(n, max(n // 300, 1), replace=False)
        v[k] = rng.integers(1, 1 << 32, len(k), dtype=np.uint64).astype(np.uint32)
        return v
    if kind == "plateaus":                   # long constant stretches: every step adds the same value to a growing float
        levels = np.array([3_000_001, 16_777_217, 16_777_215, 123_456_789, 5, 0, 999_999, 4_294_967_295], np.uint32)
        runs = rng.integers(50, 5000, n // 50 + 2)
        v = np.repeat(levels[rng.integers(0, len(levels), len(runs))], runs)
        return v[:n].astype(np.uint32)
    if kind == "sawtooth":
        return ((np.arange(n, dtype=np.uint64) % 4099) * 8191).astype(np.uint32)
    if kind == "around_2p24":                # 2^24 and its neighbours: the first integers a float cannot hold
        return (np.int64(1 << 24) + rng.integers(-2, 4, n)).astype(np.uint32)
    if kind == "uniform_u32":                # nearly every conversion rounds
        return rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    if kind == "near_u32_max":
        return (np.uint64(0xFFFFFFFF) - rng.integers(0, 300, n).astype(np.uint64)).astype(np.uint32)
    if kind == "pileup":                     # a background of tens of reads and peaks of up to a few million
        x = np.arange(n, dtype=np.float64)
        v = rng.poisson(30, n).astype(np.float64)
        for _ in range(max(n // 20000, 3)):
            c, w, h = rng.random() * n, rng.uniform(100, 3000), 10 ** rng.uniform(3, 6.6)
            lo, hi = max(int(c - 6 * w), 0), min(int(c + 6 * w) + 1, n)
            v[lo:hi] += h * np.exp(-((x[lo:hi] - c) / w) ** 2)
        return v.astype(np.uint32)
    raise ValueError(kind)


PILEUP_OPTS = ["-w", "-Q", "0"]
PILEUP_FILES = ["chrom.sizes", "rep.sizes", "rmsk.txt", "reads.bam"]


def write_pileup_input(directory, n_reads=400_000):
    """A seeded pile-up: n_reads reads over 120 copies of two repeat names on one 60 kb chromosome, so a consensus
    base is covered thousands of times and a consensus's bases sum past 2^24. Writes PILEUP_FILES into `directory`."""
    chroms = [("chr1", 60_000)]
    t = synth.make_table(8801, chroms, 120, n_names=2, n_fams=2, n_clas=2, missing_len_frac=0.0)
    r = synth.make_reads(8802, chroms, n_reads, read_len=(60, 150), unmapped_frac=0.0, odd_cigar_frac=0.02, nocigar_frac=0.0)
    d = str(directory)
    synth.write_sizes(os.path.join(d, "chrom.sizes"), chroms)
    synth.write_sizes(os.path.join(d, "rep.sizes"), t.rep_len.items())
    synth.write_rmsk(os.path.join(d, "rmsk.txt"), t)
    synth.write_bam(os.path.join(d, "reads.bam"), r, with_seq=False)
    return [os.path.join(d, f) for f in PILEUP_FILES]


def wig_depth(vals_by_name, names_in_id_order, reductions):
    """How deep a wig is, by bwfold: (level-0 summaries with sum_squares > 2^24, summaries of any level with
    sum_data > 2^24)."""
    import bwfold
    cov = np.concatenate([vals_by_name[n] for n in names_in_id_order]).astype(np.uint32)
    seqs, at = [], 0
    for n in names_in_id_order:
        seqs.append((at, len(vals_by_name[n])))
        at += len(vals_by_name[n])
    lv = bwfold.summaries(cov, seqs, reductions)
    return int((lv[0]["sum_squares"] > 2.0 ** 24).sum()), int(sum((x["sum_data"] > 2.0 ** 24).sum() for x in lv))
