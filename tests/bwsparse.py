"""What `filter -W` must write, stated apart from the code under test (tests/test_bigwig_bedgraph_writer.py,
tests/test_gpu_gcov_bigwig.py, tests/test_gpu_gcov_bigwig_cli.py).

1. `decode(data)`: a bigWig into what it says, whatever deflated its blocks; sections of type 1 (bedGraph) are accepted, which
   refio.bigwig_decode refuses. `digest(decoded)` is a sha256 over all of it.
2. `model(items, sizes)`: the decoded content the reference's converter gives for bedGraph items, from the rule alone:
   chromosomes with an item get ids in byte order of their names; sections of 1024 items; the first reduction found by reducing
   and looking at the size; further levels x4 from the last level kept; summaries that start where the data starts, re-anchor
   after a gap of a whole reduction behind the open summary's end, and take of an item that a boundary cuts the fraction
   overlap / REMAINING length (not its length): the part of the item in front of the boundary has been given away when the
   divisor is taken.
3. the cases of the GPU tests, their recorded digests (tests/golden/gcov_bigwig/digests.json; python tests/bwsparse.py --record
   where oracle/_ref/libcuskent.a exists), and `reference_bigwig`, which runs the reference's bigWigFileCreate through a driver
   of a few lines."""
import hashlib
import json
import os
import shutil
import struct
import subprocess
import sys
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARCHIVE = os.path.join(ROOT, "oracle", "_ref", "libcuskent.a")
GOLDEN = os.path.join(ROOT, "tests", "golden", "gcov_bigwig", "digests.json")
PER_SLOT = 1024


# ---- 1. the decoder

def decode(data: bytes):
    sig, version, n_zoom, chrom_off, data_off, index_off, fcnt, dfcnt, asql, total_off, unc_buf, _ = struct.unpack_from("<IHHQQQHHQQIQ", data, 0)
    assert sig == 0x888FFC26 and struct.unpack_from("<I", data, len(data) - 4)[0] == sig
    zooms = [struct.unpack_from("<IIQQ", data, 64 + 24 * i) for i in range(n_zoom)]
    total = struct.unpack_from("<Qdddd", data, total_off) if total_off else None
    magic, bsize, ksize, vsize, n_chrom, _ = struct.unpack_from("<IIIIQQ", data, chrom_off)
    assert magic == 0x78CA8C91 and vsize == 8
    chroms = []

    def bpt(off):
        leaf, _, cnt = struct.unpack_from("<BBH", data, off)
        for i in range(cnt):
            at = off + 4 + i * (ksize + 8)
            key = data[at:at + ksize].split(b"\0", 1)[0].decode()
            if leaf:
                chroms.append((key,) + struct.unpack_from("<II", data, at + ksize))
            else:
                bpt(struct.unpack_from("<Q", data, at + ksize)[0])
    bpt(chrom_off + 32)
    assert len(chroms) == n_chrom

    def cir(off):
        magic, bs, cnt, sc, sb, ec, eb, end_off, per_slot, _ = struct.unpack_from("<IIQIIIIQII", data, off)
        assert magic == 0x2468ACE0
        out = []

        def rec(o):
            leaf, _, n = struct.unpack_from("<BBH", data, o)
            for i in range(n):
                if leaf:
                    out.append(struct.unpack_from("<IIIIQQ", data, o + 4 + 32 * i))
                else:
                    rec(struct.unpack_from("<Q", data, o + 4 + 24 * i + 16)[0])
        rec(off + 48)
        return (bs, cnt, (sc, sb, ec, eb), per_slot), out

    n_sections, = struct.unpack_from("<Q", data, data_off)
    head, leaves = cir(index_off)
    sections = []
    for sc, sb, ec, eb, off, size in leaves:
        raw = zlib.decompress(data[off:off + size])
        cid, start, end, step, span, typ, res, cnt = struct.unpack_from("<IIIIIBBH", raw, 0)
        assert (sc, sb, ec, eb) == (cid, start, cid, end)
        assert typ in (1, 3) and len(raw) == 24 + (12 if typ == 1 else 4) * cnt
        sections.append((cid, start, end, step, span, typ, res, cnt, raw[24:]))
    assert len(sections) == n_sections == head[1]
    zoom_out = []
    for red, _, zdata, zindex in zooms:
        cnt, = struct.unpack_from("<I", data, zdata)
        zh, zl = cir(zindex)
        recs = b"".join(zlib.decompress(data[off:off + size]) for _, _, _, _, off, size in zl)
        assert len(recs) == 32 * cnt == 32 * zh[1]
        zoom_out.append((red, zh, recs))
    return {"version": version, "field_counts": (fcnt, dfcnt, asql), "uncompress_buf": unc_buf, "total": total, "chroms": chroms,
            "chrom_tree": (bsize, ksize), "index": head, "sections": sections, "zooms": zoom_out}


def digest(d) -> str:
    """sha256 over what a file says: chromosomes, key size and block size of their tree, the sections, every level's reduction and
    records, the total summary and the uncompress buffer size. (Not the shape of the R trees: decode() walks them, and the command
    tests compare whole decoded files.)"""
    h = hashlib.sha256()
    h.update(repr((d["uncompress_buf"], d["total"], d["chroms"], d["chrom_tree"])).encode())
    for s in d["sections"]:
        h.update(struct.pack("<IIIIIBBH", *s[:8]) + s[8])
    for z in d["zooms"]:
        h.update(struct.pack("<I", z[0]) + z[-1])
    return h.hexdigest()


def model_as_decoded(m):
    """the model in the form digest() takes"""
    return {"uncompress_buf": m["uncompress_buf"], "total": m["total"], "chroms": m["chroms"],
            "chrom_tree": (min(256, len(m["chroms"])), max(len(n) for n, _, _ in m["chroms"])), "sections": m["sections"], "zooms": m["zooms"]}


def from_result(res, names, sizes):
    """what engine.Gcov.bigwig() hands out (the C ABI's content, before a file exists) in the form decode() gives: every block is
    inflated here; names / sizes: the chromosomes as the coverage object was created with them"""
    chroms = [(names[int(c)], i, int(sizes[int(c)])) for i, c in enumerate(res["chrom"])]
    sections = []
    for i, (key, cnt) in enumerate(zip(res["sec_key"], res["sec_count"])):
        raw = zlib.decompress(res["blocks"][i])
        head = struct.unpack_from("<IIIIIBBH", raw, 0)
        assert head[:3] == tuple(int(x) for x in key) and head[7] == cnt and len(raw) == 24 + 12 * cnt
        sections.append(head + (raw[24:],))
    zooms = []
    ends = list(res["slot_first"][1:]) + [len(res["blocks"])]
    assert res["slot_first"][0] == len(sections)
    for red, recs, a, b in zip(res["reductions"], res["sums"], res["slot_first"], ends):
        assert b - a == (len(recs) // 32 + PER_SLOT - 1) // PER_SLOT
        assert b"".join(zlib.decompress(x) for x in res["blocks"][a:b]) == recs, "the zoom blocks do not inflate to the summaries"
        zooms.append((red, recs))
    first = [struct.unpack_from("<IIIIffff", zooms[0][1], k) for k in range(0, len(zooms[0][1]), 32)]
    total = (sum(r[3] for r in first), min(r[4] for r in first), max(r[5] for r in first), _sum_in_order(first, 6), _sum_in_order(first, 7))
    return {"uncompress_buf": max(32 * PER_SLOT, max(24 + 12 * s[7] for s in sections)), "total": total, "chroms": chroms,
            "chrom_tree": (min(256, len(chroms)), max(len(n) for n, _, _ in chroms)), "sections": sections, "zooms": zooms}


def items_of(d):
    """the decoded sections back as {chromosome name: [(start, end, float32 value)]}"""
    names = {cid: nm for nm, cid, _ in d["chroms"]}
    out = {}
    for cid, _, _, _, _, typ, _, cnt, raw in d["sections"]:
        assert typ == 1
        a = np.frombuffer(raw, "<u4").reshape(-1, 3)
        out.setdefault(names[cid], []).extend(zip(a[:, 0].tolist(), a[:, 1].tolist(), a[:, 2].view("<f4").tolist()))
    return out


# ---- 2. the model

def _f32(x):
    return float(np.float32(x))


def chain(items, sizes, red):
    """items: (chrom id, start, end, valid count, min, max, sum, sum of squares), in order -> the summaries, as lists of the same
    eight. The float fields hold float32 values; what is added to them is rounded to float32 after every step, in double before."""
    out, cur = [], None
    for c, s, e, vc, mn, mx, sd, sq in items:
        e = min(e, sizes[c])
        while s < e:
            if cur is None or cur[0] != c or cur[2] <= s:
                st = s if (cur is None or cur[0] != c or cur[2] + red <= s) else cur[2]
                cur = [c, st, min(st + red, sizes[c]), 0, _f32(mn), _f32(mx), 0.0, 0.0]
                out.append(cur)
            ov = min(e, cur[2]) - max(s, cur[1])
            f = ov / (e - s)                                  # s has moved on: the divisor is what is LEFT of the item
            cur[3] = int(cur[3] + f * vc) & 0xffffffff
            if cur[4] > mn:
                cur[4] = _f32(mn)
            if cur[5] < mx:
                cur[5] = _f32(mx)
            cur[6] = _f32(cur[6] + f * sd)
            cur[7] = _f32(cur[7] + f * sq)
            s += ov
    return out


MAX_RED = 0x3fffffff                                      # the reference's BIGNUM: no reduction above it (or below 1) is counted


def zoom_levels(full, min_res, n_chrom, count):
    """which zoom levels a file gets, from counts alone. full: the bytes of all sections' payloads; min_res: the mean of the sections'
    smallest item lengths; count(red, src): the summaries reduction `red` gives over the data (src None) or over the level of
    reduction `src`. -> tries (the first reductions counted), refused (the first reduction that was outside 1 .. MAX_RED, or None),
    levels (the reductions kept), dropped (refused by the size comparison), steps [(reduction, the level it was counted from, kept)]"""
    red, last, tries = min_res * 10, 0, []
    out = {"tries": tries, "refused": None, "levels": [], "dropped": [], "steps": []}
    while True:
        if not 1 <= red <= MAX_RED:
            out["refused"] = red
            return out
        n = count(red, None)
        tries.append(red)
        size = 2 * 32 * n
        if size >= full // 2 and size != last:
            red = max(int(1.1 * red * size / (full // 2)), 2 * red)
            last = size
        else:
            break
    out["levels"].append(red)
    for _ in range(9):
        red *= 4
        if red > 1000000000:
            break
        src = out["levels"][-1]
        n = count(red, src)
        keep = 32 * n != last
        out["levels" if keep else "dropped"].append(red)
        out["steps"].append((red, src, keep))
        if n <= n_chrom:
            break
    return out


def pack_summaries(v):
    return b"".join(struct.pack("<IIIIffff", *r) for r in v)


def model(items, sizes):
    """items: {chromosome name: [(start, end, value)]} (starts ascending, no overlap), sizes: {name: size} -> what decode() gives for
    the reference's file, less the tree shapes: chroms, sections, zooms [(reduction, records)], uncompress_buf, total; and how the
    levels were found: rounds (first-reduction tries), dropped (reductions refused by the size comparison)"""
    names = sorted((n for n in items if items[n]), key=lambda n: n.encode())
    assert names, "no data: the converter refuses"
    cid = {n: i for i, n in enumerate(names)}
    size_of = [sizes[n] for n in names]
    chroms = [(n, cid[n], sizes[n]) for n in names]
    sections, level0, res_sum, full = [], [], 0, 0
    for n in names:
        v = [(int(s), int(e), _f32(x)) for s, e, x in items[n]]
        for k in range(0, len(v), PER_SLOT):
            part = v[k:k + PER_SLOT]
            raw = b"".join(struct.pack("<IIf", *p) for p in part)
            sections.append((cid[n], part[0][0], part[-1][1], 0, 0, 1, 0, len(part), raw))
            res_sum += min(e - s for s, e, _ in part)
            full += 24 + 12 * len(part)
        for s, e, x in v:
            size = e - s
            level0.append((cid[n], s, e, size, x, x, size * x, (size * x) * x))
    n_sec = len(sections)
    made = {}

    def count(red, src):
        made[red] = chain(level0 if src is None else made[src], size_of, red)
        return len(made[red])
    z = zoom_levels(full, (res_sum + n_sec // 2) // n_sec, len(names), count)
    assert z["refused"] is None, z
    zooms, rounds, dropped = [(r, made[r]) for r in z["levels"]], len(z["tries"]), z["dropped"]
    first = zooms[0][1]
    total = (sum(r[3] for r in first), min(r[4] for r in first), max(r[5] for r in first), _sum_in_order(first, 6), _sum_in_order(first, 7))
    return {"chroms": chroms, "sections": sections, "zooms": [(r, pack_summaries(v)) for r, v in zooms], "total": total,
            "uncompress_buf": max(32 * PER_SLOT, max(24 + 12 * s[7] for s in sections)), "rounds": rounds, "dropped": dropped}


def _sum_in_order(v, k):
    t = v[0][k]
    for r in v[1:]:
        t += r[k]
    return t


def check_against_model(d, m):
    """the decoded file d says what the model m says"""
    assert d["chroms"] == m["chroms"]
    assert d["chrom_tree"] == (min(256, len(m["chroms"])), max(len(n) for n, _, _ in m["chroms"]))
    assert d["uncompress_buf"] == m["uncompress_buf"]
    assert len(d["sections"]) == len(m["sections"])
    for a, b in zip(d["sections"], m["sections"]):
        assert a == b, (a[:8], b[:8])
    assert [z[0] for z in d["zooms"]] == [z[0] for z in m["zooms"]], "reductions"
    for z, (red, want) in zip(d["zooms"], m["zooms"]):
        recs = z[-1]
        if recs != want:
            k = next(i for i in range(0, max(len(recs), len(want)), 32) if recs[i:i + 32] != want[i:i + 32])
            raise AssertionError(f"reduction {red}: record {k // 32} of {len(recs) // 32} / {len(want) // 32}: "
                                 f"{struct.unpack('<IIIIffff', recs[k:k + 32]) if k + 32 <= len(recs) else None} != "
                                 f"{struct.unpack('<IIIIffff', want[k:k + 32]) if k + 32 <= len(want) else None}")
    assert d["total"] == m["total"]


def bedgraph_text(items):
    out = []
    for n in sorted(items, key=lambda n: n.encode()):
        for s, e, x in items[n]:
            out.append("%s\t%d\t%d\t%d\n" % (n, s, e, x) if float(x).is_integer() else "%s\t%d\t%d\t%r\n" % (n, s, e, float(x)))
    return "".join(out)


def parse_bedgraph(text):
    items = {}
    for line in text.splitlines():
        c = line.split("\t")
        items.setdefault(c[0], []).append((int(c[1]), int(c[2]), float(c[3])))
    return items


# ---- 3. the reference, the cases, the recording

DRIVER = """
void bigWigFileCreate(char *inName, char *chromSizes, int blockSize, int itemsPerSlot, int clipDontDie, int compress, char *outName);
int main(int argc, char **argv)
{
    if (argc != 4) return 2;
    bigWigFileCreate(argv[1], argv[2], 256, 1024, 0, 1, argv[3]);
    return 0;
}
"""


def have_reference():
    return os.path.exists(ARCHIVE) and shutil.which("gcc") is not None


def build_driver(workdir):
    src, exe = os.path.join(workdir, "bw_ref_driver.c"), os.path.join(workdir, "bw_ref_driver")
    if not os.path.exists(exe):
        with open(src, "w") as f:
            f.write(DRIVER)
        subprocess.check_call(["gcc", "-O1", "-o", exe, src, ARCHIVE, "-pthread", "-lm", "-lz"])
    return exe


def write_inputs(workdir, items, sizes, stem="in"):
    bg, cs = os.path.join(workdir, stem + ".bedGraph"), os.path.join(workdir, stem + ".sizes")
    with open(bg, "w") as f:
        f.write(bedgraph_text(items))
    with open(cs, "w") as f:
        f.write("".join(f"{n}\t{s}\n" for n, s in sizes.items()))
    return bg, cs


def reference_bigwig(workdir, bedgraph, chrom_sizes, out):
    pr = subprocess.run([build_driver(workdir), bedgraph, chrom_sizes, out], capture_output=True, text=True, timeout=600)
    return pr


def depth_items(intervals):
    """[(start, end)] on one chromosome -> the bedGraph items of their depth: [(start, end, depth)]"""
    a = np.asarray(intervals, np.int64).reshape(-1, 2)
    pos, inv = np.unique(np.concatenate([a[:, 0], a[:, 1]]), return_inverse=True)
    diff = np.zeros(len(pos), np.int64)
    np.add.at(diff, inv, np.concatenate([np.ones(len(a), np.int64), -np.ones(len(a), np.int64)]))
    keep = diff != 0
    pos, depth = pos[keep], np.cumsum(diff[keep])
    return [(int(pos[k]), int(pos[k + 1]), float(depth[k])) for k in range(len(pos) - 1) if depth[k] > 0]


def blocks(rng, n, start, gap_max, len_max=40, depth_max=4, end_before=None):
    """n separate stretches from `start` on: random lengths, random gaps in [1, gap_max], each stretch one or more stacked reads ->
    intervals whose depth gives at least n items"""
    out, at = [], start
    for _ in range(n):
        ln = int(rng.integers(1, len_max + 1))
        for _ in range(int(rng.integers(1, depth_max + 1))):
            out.append((at, at + ln))
        at += ln + int(rng.integers(1, gap_max + 1))
    assert end_before is None or at < end_before
    return out


def exact_items(k, start, length=3, gap=2):
    """k intervals that give exactly k items (apart, one read each)"""
    return [(start + i * (length + gap), start + i * (length + gap) + length) for i in range(k)]


def recorded():
    with open(GOLDEN) as f:
        return json.load(f)


if __name__ == "__main__" and "--record" in sys.argv:
    import tempfile
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import gcovbwcases
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        for key, (sizes, per_file) in gcovbwcases.all_cases().items():
            for w, items in enumerate(per_file):
                if not any(items.values()):
                    continue
                bg, cs = write_inputs(tmp, items, sizes, f"{key}_{w}")
                bw = os.path.join(tmp, f"{key}_{w}.bw")
                pr = reference_bigwig(tmp, bg, cs, bw)
                assert pr.returncode == 0, pr.stderr
                out[f"{key}/{w}"] = digest(decode(open(bw, "rb").read()))
                print(key, w, out[f"{key}/{w}"][:16])
    os.makedirs(os.path.dirname(GOLDEN), exist_ok=True)
    with open(GOLDEN, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
