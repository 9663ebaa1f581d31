"""The reference's own BAM library as a checker: oracle/_ref/bamcheck (oracle/bamcheck.c over the samtools 0.1.18 the reference
vendors) run on files in the product's layout, and its answers compared with the restatements of tests/baicase.py.

  library_index(path)          the bytes bam_index_build writes for the file
  normalise(lib, ours)         the library's parsed index with the two documented differences taken to ours, each under its condition
  check_index(path, ours)      the library's index of the file equals `ours` byte for byte after normalise and with bins ascending
  check_fetch(path, bai, regions)   bam_fetch through `bai` returns the records of baicase.linear_scan, region by region
  view(path)                   (header lines, record lines) of the file as the library prints them
  library_sort(path, out)      the records of the file after bam_sort_core, one by one

DESIGN.md ("The index against the reference's own indexer") derives the differences from bam_index.c."""
import os
import struct
import subprocess

import numpy as np

import baicase as bai
import refio

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAMCHECK = os.path.join(ROOT, "oracle", "_ref", "bamcheck")
present = os.path.exists(BAMCHECK)


def run(*args):
    pr = subprocess.run([BAMCHECK] + [str(a) for a in args], capture_output=True, timeout=120)
    assert pr.returncode == 0, (args, pr.stderr[-1000:])
    return pr


def library_index(path):
    """(bam_index_build writes <path>.bai: a .bai of ours beside the file is read before and put back by the caller)"""
    run("index", path)
    with open(str(path) + ".bai", "rb") as f:
        return f.read()


def bai_bytes(refs):
    """parse_bai's structure back to bytes: a reference's bins ascending, its pseudo-bin behind them"""
    out = [b"BAI\1", struct.pack("<i", len(refs))]
    for r in refs:
        out.append(struct.pack("<i", len(r["bins"]) + (r["meta"] is not None)))
        for bn in sorted(r["bins"]):
            out.append(struct.pack("<Ii", bn, len(r["bins"][bn])) + b"".join(struct.pack("<QQ", *c) for c in r["bins"][bn]))
        if r["meta"] is not None:
            out.append(struct.pack("<IiQQQQ", bai.PSEUDO, 2, *r["meta"]))
        out.append(struct.pack("<i%dQ" % len(r["lin"]), len(r["lin"]), *r["lin"]))
    return b"".join(out) + bytes(8)


def normalise(lib, ours):
    """lib, ours: parse_bai's lists. Two places of `lib` are taken to ours, each only under its condition:
    1. the end of the file's last chunk (bam_tell after the read that met the end of the file) and the pseudo-bin end that is the
       same number: only in the last reference with records, only where it is a virtual offset at or beyond ours;
    2. a linear index that ends with the window of the reference's last record: only shorter than ours, ours fills what lacks."""
    lib = [{"bins": {bn: list(ch) for bn, ch in r["bins"].items()}, "meta": r["meta"], "lin": list(r["lin"])} for r in lib]
    with_records = [t for t, r in enumerate(ours) if r["meta"] is not None]
    if with_records and lib[with_records[-1]]["meta"] is not None:
        r, end = lib[with_records[-1]], ours[with_records[-1]]["meta"][1]
        lib_end = r["meta"][1]
        assert lib_end >= end, (lib_end, end)
        at = [bn for bn, ch in r["bins"].items() if ch[-1][1] == lib_end]
        assert len(at) == 1, at
        r["bins"][at[0]][-1] = (r["bins"][at[0]][-1][0], end)
        r["meta"] = (r["meta"][0], end) + r["meta"][2:]
    for r, o in zip(lib, ours):
        assert len(r["lin"]) <= len(o["lin"])
        r["lin"] += o["lin"][len(r["lin"]):]
    return lib


def check_index(path, ours):
    """the library's index of the file at `path` against the index bytes `ours`; returns the library's parsed index as it wrote it"""
    lib = bai.parse_bai(library_index(path))
    assert bai_bytes(normalise(lib, bai.parse_bai(ours))) == ours
    return lib


def view(path):
    text = run("view", path).stdout.split(b"\n")
    assert text.pop() == b""
    head = [ln for ln in text if ln.startswith(b"@")]
    assert text[:len(head)] == head
    return head, text[len(head):]


def check_fetch(path, bai_data, regions):
    """bam_fetch of every (tid, beg, end) through the index bytes `bai_data`, written beside the file, against the linear scan of
    the file's records; the records are told apart by their SAM lines. Returns how many regions held a record"""
    with open(str(path) + ".bai", "wb") as f:
        f.write(bai_data)
    with open(path, "rb") as f:
        l_ref, stream, sizes, first, raw, ustart = bai.split_bam(f.read())
    start = len(raw) - len(stream)
    recs = bai.records_of(stream)
    lines = view(path)[1]
    assert len(lines) == len(recs)
    r_tid, r_pos, r_end, r_at, _ = np.array(recs, np.int64).reshape(-1, 5).T    # the linear scan: every record against the region
    hits = 0
    for k, (tid, beg, end) in enumerate(regions):
        got = run("fetch", path, tid, beg, end).stdout.split(b"\n")
        assert got.pop() == b""
        want = np.flatnonzero((r_tid == tid) & (r_pos < end) & (r_end > beg))
        if k % 16 == 0:                                                    # (baicase.linear_scan walks the bytes: the same set, slowly)
            assert {start + int(r_at[i]) for i in want} == bai.linear_scan(raw, start, tid, beg, end)
        assert sorted(got) == sorted(lines[i] for i in want), (tid, beg, end)
        hits += bool(len(want))
    return hits


def edge_regions(path):
    """regions for check_fetch from the file's own records: the first, the middle and the last record of every reference with one
    base on either side of its start, of its end and of the 16 KiB window and 128 KiB bin edges next to it; every whole reference
    (the empty ones too); the stretch behind the last record"""
    with open(path, "rb") as f:
        l_ref, stream = bai.split_bam(f.read())[:2]
    recs = bai.records_of(stream)
    out = []
    for tid, ln in enumerate(l_ref[:8]):
        out.append((tid, 0, max(ln, 1)))
        mine = [r for r in recs if r[0] == tid]
        if not mine:
            continue
        last = max(r[2] for r in mine)
        out.append((tid, last, last + 1000))
        for r in (mine[0], mine[len(mine) // 2], mine[-1]):
            out += [(tid, max(r[1] - 1, 0), r[1] or 1), (tid, r[1], r[1] + 1), (tid, r[2] - 1, r[2]), (tid, r[2], r[2] + 1)]
            for shift in (14, 17):
                for edge in {r[1] >> shift << shift, ((r[2] - 1) >> shift) + 1 << shift}:
                    out += [(tid, max(edge - 1, 0), edge or 1), (tid, edge, edge + 1), (tid, max(edge - 1, 0), edge + 1)]
    keep = []
    for reg in out:
        if reg not in keep:
            keep.append(reg)
    return keep


def library_sort(path, prefix):
    """the records of <prefix>.bam, which bam_sort_core makes of the file, one by one, and the header's bytes"""
    run("sort", path, prefix)
    raw = refio.bgzf_decompress(open(str(prefix) + ".bam", "rb").read())
    l_text, = struct.unpack_from("<i", raw, 4)
    at = 8 + l_text
    n_ref, = struct.unpack_from("<i", raw, at)
    at += 4
    for _ in range(n_ref):
        at += 8 + struct.unpack_from("<i", raw, at)[0]
    head, recs = raw[:at], []
    while at < len(raw):
        bs, = struct.unpack_from("<I", raw, at)
        recs.append(raw[at:at + 4 + bs])
        at += 4 + bs
    assert at == len(raw)
    return head, recs
