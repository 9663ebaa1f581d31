"""csrc/itx_bigwig.hip and csrc/itx_deflate_core.h through the C ABI (itx_bigwig_start / collect), held to tests/bwfold.py
(the plain numpy restatement of the sections and of bbiAddToSummary's sequential float fold) and to the one-lane host
build of the encoder (tests/deflate_host.cpp), bit for bit.

Chosen coverage gets into the engine through itx_engine_finish_partial: a stat table whose rows all carry one
(repName, repFamily, repClass) has one unit as long as the consensus, and the u32 part of a partial is the two coverage
difference arrays, so D = diff(wanted coverage) mod 2^32 makes k_finish_unit's carried scan return the wanted vector
(asserted first: a scan over a unit of millions of slots whose values wrap). The sequences of a bigWig are then arbitrary
(offset, length) windows of that vector, so content and geometry are chosen independently:

  content   bwcases.CONTENT, one class for "all" and another for "unique": the exact regime, spikes, plateaus, a sawtooth,
            2^24 and its neighbours, uniform uint32, values next to 2^32 - 1, a pile-up with peaks of millions
  geometry  GEOMETRY below: lengths around 1, the section size and the reductions; r0 of 1, 2, 10, 34, 1000; ratios 4, 16
            and 64; 0, 1 and 10 levels; no sequence at all; one sequence of 1.2 M bases (35 zoom blocks at level 0, more
            than 1024 blocks: k_size_scan gives a thread several); 2500 short sequences; offsets unordered, with gaps and
            overlaps

Every (content, geometry) pair is a case; each is checked for uniq 0 and 1: the counts, every block inflating to the
payload and ending where its stream ends, the summaries as raw bytes, every block's compressed bytes equal to the host
build's (itx_deflate_core.h: "the host and device builds give the same bytes"), and a second build the same. What a case
is there FOR (stored and dynamic blocks of both kinds, folds whose order matters) is asserted on the expected data."""
import ctypes as C
import zlib

import numpy as np
import pytest

import bwcases
import bwfold
import deflatehost
from iteres_amd import engine as eng

pytestmark = pytest.mark.gpu

COV_LEN = 2_300_000
E_ARG, E_STATE = -1, -5                  # include/iteres_amd.h


def _place(rng, lengths):
    """windows anywhere in the coverage: not in order, with gaps, overlapping where they fall so"""
    return [(int(rng.integers(0, COV_LEN - n + 1)), int(n)) for n in lengths]


def _around(r0):
    return [n for n in (1, 2, 1023, 1024, 1025, r0 - 1, r0, r0 + 1, 1024 * r0, 1024 * r0 + 1) if n >= 1]


GEOMETRY = {
    # name: (lengths in id order, reductions)
    "r1_ten_levels": (_around(1) + [300_000, 5], [4 ** k for k in range(10)]),
    "r2_ratios_16_64": (_around(2) + [5000], [2, 32, 2048]),
    "r10_ratios_4_16_64": (_around(10) + [70_001], [10, 40, 640, 40960]),
    "r34_ratios_4_16_64": (_around(34), [34, 136, 2176, 139264]),
    "r1000_ratios_64_4": (_around(1000), [1000, 64000, 256000]),
    "one_long_sequence": ([3, 1_200_007, 1024], [34, 136, 544, 2176]),
    "many_short_sequences": (lambda rng: [int(x) for x in rng.integers(1, 41, 2500)], [10, 40, 160]),
    "tiny_sections": ([8, 64, 1, 2, 3, 8, 64, 16], [34]),          # sections of 56 and 280 bytes, a zoom block of 8 summaries
    "one_base": ([1], [1000, 4000]),
    "one_summary_zoom_block": ([34 * 1024, 20], [34, 136]),        # level 0: a full zoom block, then one of a single summary
    "no_levels": ([1, 1024, 1025, 7], []),
    "one_level": ([1, 1024, 1025, 50_000], [34]),
    "no_sequence": ([], [10, 40, 160]),
}


def _geometry(name):
    rng = np.random.default_rng([77, list(GEOMETRY).index(name)])
    lengths, reds = GEOMETRY[name]
    if callable(lengths):
        lengths = lengths(rng)
    return _place(rng, lengths), list(reds)


# what a pair is there for (asserted on the expected payloads and the host encoder's output, never on the device's):
#   stored_*        a section / a zoom block takes the stored form
#   dynamic_full_*  a section of 4120 bytes / a zoom block of 32768 bytes is a dynamic block
#   order           (float)cov != cov somewhere, a level-0 sum_data differs from the float64 sum of its bases, and a
#                   sum_data of level 1 differs from the float64 sum of its inputs
REQUIRED = {
    ("uniform_u32", "tiny_sections"): {"stored_section"},
    ("uniform_u32", "one_summary_zoom_block"): {"stored_zoom", "dynamic_full_zoom"},
    ("small", "one_long_sequence"): {"dynamic_full_section", "dynamic_full_zoom"},
    ("pileup", "one_long_sequence"): {"dynamic_full_section", "dynamic_full_zoom"},
    ("uniform_u32", "r34_ratios_4_16_64"): {"order"},
    ("uniform_u32", "one_long_sequence"): {"order"},
    ("near_u32_max", "r10_ratios_4_16_64"): {"order"},
}

TOTALS = {"builds": 0, "blocks": 0, "summaries": 0, "device_ms": 0.0}


class Rig:
    """one table (a single consensus of COV_LEN bases), one stat engine, the host encoder"""

    def __init__(self, tmp):
        import torch
        self.torch = torch
        self.dev = torch.device("cuda", 0)
        self.enc = deflatehost.build_encoder(tmp)
        n = 6
        rows = eng.make_rows([0] * n, [1000 * i for i in range(n)], [1000 * i + 500 for i in range(n)], [0] * n, [500] * n, [0] * n, [0] * n, [0] * n)
        self.table = eng.Table(rows, np.array([10_000_000], np.int64), np.array([COV_LEN], np.uint32), 1, 1)
        self.engine = eng.Engine(self.table, {}, batch_capacity=1 << 12)
        self.engine.set_tidmap([0])
        self.loaded = None
        self.cov = None

    def load(self, kind):
        """the engine's coverage becomes content `kind` (all reads) and another class (unique reads)"""
        if self.loaded == kind:
            return self.cov
        torch = self.torch
        i = bwcases.CONTENT.index(kind)
        want = [bwcases.content(kind, COV_LEN, 500 + i), bwcases.content(bwcases.CONTENT[(i + 3) % len(bwcases.CONTENT)], COV_LEN, 900 + i)]
        assert not np.array_equal(want[0], want[1])
        info = self.table.info
        n64, n32 = self.engine.partial_size()
        assert int(info.cov_len) == COV_LEN and n64 == 16 + 2 * int(info.n_units) and n32 == 2 * int(info.n_slots)
        assert int(info.n_units) == 1 and int(info.n_slots) == COV_LEN + 1, "one triple, one unit: the consensus and its extra slot"
        d32 = np.zeros(n32, np.uint32)
        for u, w in enumerate(want):
            d = np.empty(COV_LEN + 1, np.uint32)
            d[0] = w[0]
            d[1:COV_LEN] = w[1:] - w[:-1]                          # uint32 arithmetic: mod 2^32
            d[COV_LEN] = (0 - int(w[-1])) & 0xFFFFFFFF             # the slot past the consensus: no part of the coverage
            d32[u * (COV_LEN + 1):(u + 1) * (COV_LEN + 1)] = d
        p64 = torch.zeros(n64, dtype=torch.int64, device=self.dev)
        p32 = torch.from_numpy(d32.view(np.int32)).to(self.dev)
        torch.cuda.synchronize()
        res = self.engine.finish_partial(p64.data_ptr(), p32.data_ptr())
        # k_finish_unit's scan, carried over 8985 rounds of 256 slots, with values that wrap
        for key, w in (("cov", want[0]), ("cov_uniq", want[1])):
            assert np.array_equal(res[key], w), f"{kind}: {key} differs first at {int(np.flatnonzero(res[key] != w)[0])}"
        self.loaded, self.cov = kind, want
        return want

    def close(self):
        self.engine.close()
        self.table.close()


@pytest.fixture(scope="module")
def rig(tmp_path_factory):
    r = Rig(tmp_path_factory.mktemp("bwk"))
    yield r
    r.close()
    print(f"\nbigWig kernels: {TOTALS['builds']} builds compared, {TOTALS['blocks']} blocks, {TOTALS['summaries']} summaries, "
          f"device_ms {TOTALS['device_ms']:.1f} (information only)")


def _properties(cov, seqs, reds, want, host_sec, host_zoom):
    """what the EXPECTED data of a build shows (see REQUIRED)"""
    props = set()
    if any(c[2] & 7 == 1 for c in host_sec):
        props.add("stored_section")
    if any(c[2] & 7 == 1 for z in host_zoom for c in z):
        props.add("stored_zoom")
    if any(len(p) == 4120 and c[2] & 7 == 5 for p, c in zip(want["sections"], host_sec)):
        props.add("dynamic_full_section")
    if any(len(p) == 32768 and c[2] & 7 == 5 for zp, zc in zip(want["zoom"], host_zoom) for p, c in zip(zp, zc)):
        props.add("dynamic_full_zoom")
    if len(reds) >= 2 and seqs:
        raw = np.concatenate([cov[o:o + n] for o, n in seqs]).astype(np.float64)
        vals = bwfold.base_values(raw.astype(np.uint32)).astype(np.float64)
        l0, l1 = want["levels"][0], want["levels"][1]
        lens = np.array([n for _, n in seqs], np.int64)
        vbase = np.concatenate([[0], np.cumsum(lens)])
        exact0 = np.add.reduceat(vals, vbase[l0["chrom_id"]] + l0["start"]).astype(np.float32)
        f0 = np.concatenate([[0], np.cumsum((lens + reds[0] - 1) // reds[0])])
        first1 = f0[l1["chrom_id"]] + (l1["start"].astype(np.int64) // reds[1]) * (reds[1] // reds[0])
        exact1 = np.add.reduceat(l0["sum_data"].astype(np.float64), first1).astype(np.float32)
        if (vals != raw).any() and (l0["sum_data"] != exact0).any() and (l1["sum_data"] != exact1).any():
            props.add("order")
    return props


def _check_build(rig, cov, uniq, seqs, reds, tag):
    want = bwfold.build(cov, seqs, reds)
    host_sec = [rig.enc(p) for p in want["sections"]]
    host_zoom = [[rig.enc(p) for p in z] for z in want["zoom"]]
    payloads = want["sections"] + [p for z in want["zoom"] for p in z]
    host = host_sec + [c for z in host_zoom for c in z]

    b = eng.Bigwig(rig.engine, uniq, seqs, reds)
    got = b.collect()
    b.close()
    # 1. the counts
    assert got["n_sec"] == len(want["sections"]), tag
    assert got["n_levels"] == len(reds)
    assert got["n_sum"] == [len(x) for x in want["levels"]], tag
    slot, at = [], len(want["sections"])
    for z in want["zoom"]:
        slot.append(at)
        at += len(z)
    assert got["slot_first"] == slot and got["n_blocks"] == at == len(payloads), tag
    off = got["block_off"].astype(np.int64)
    assert off[0] == 0 and (np.diff(off) > 0).all() and off[-1] == len(got["blocks"]), tag
    # 3. the summaries, as bytes
    for k, lv in enumerate(want["levels"]):
        g = got["levels"][k]
        if g.tobytes() != lv.tobytes():
            assert len(g) == len(lv)
            i = int(np.flatnonzero(g.view("V32") != lv.view("V32"))[0])
            raise AssertionError(f"{tag}: level {k} (reduction {reds[k]}), summary {i} of {len(lv)}: device {g[i]} / fold {lv[i]}")
    # 2. and 4. the blocks
    blocks = got["blocks"]
    for i, (p, h) in enumerate(zip(payloads, host)):
        c = blocks[off[i]:off[i + 1]]
        z = zlib.decompressobj()
        assert z.decompress(c) == p and z.eof and z.unused_data == b"", f"{tag}: block {i} does not inflate to its payload"
        assert c == h, f"{tag}: block {i} ({len(p)} bytes in): device {len(c)} bytes and host build {len(h)} bytes differ"
    # 5. again: the same bytes
    b = eng.Bigwig(rig.engine, uniq, seqs, reds)
    again = b.collect()
    b.close()
    assert again["blocks"] == blocks and np.array_equal(again["block_off"], got["block_off"]), f"{tag}: a second build differs"
    assert all(a.tobytes() == g.tobytes() for a, g in zip(again["levels"], got["levels"])), f"{tag}: a second build's summaries differ"
    TOTALS["builds"] += 1
    TOTALS["blocks"] += len(payloads)
    TOTALS["summaries"] += sum(len(x) for x in want["levels"])
    TOTALS["device_ms"] += got["device_ms"]
    return _properties(cov, seqs, reds, want, host_sec, host_zoom)


@pytest.mark.parametrize("geometry", list(GEOMETRY))
@pytest.mark.parametrize("kind", bwcases.CONTENT)
def test_device_build_equals_fold_and_host_encoder(rig, kind, geometry):
    cov = rig.load(kind)
    seqs, reds = _geometry(geometry)
    props = [_check_build(rig, cov[uniq], uniq, seqs, reds, f"{kind}/{geometry}/uniq={uniq}") for uniq in (0, 1)]
    missing = REQUIRED.get((kind, geometry), set()) - props[0]
    assert not missing, f"{kind}/{geometry} no longer shows {sorted(missing)}: the case has become shallow"


def test_geometry_is_what_it_claims():
    """the geometry classes, checked on the tables above"""
    for name in GEOMETRY:
        seqs, reds = _geometry(name)
        assert all(0 <= o and o + n <= COV_LEN and n >= 1 for o, n in seqs)
        assert all(r < 1 << 31 for r in reds) and all(b % a == 0 and b // a in (4, 16, 64) for a, b in zip(reds, reds[1:]))
    assert {len(_geometry(n)[1]) for n in GEOMETRY} >= {0, 1, 10}
    assert {_geometry(n)[1][0] for n in GEOMETRY if _geometry(n)[1]} >= {1, 2, 10, 34, 1000}
    assert {b // a for n in GEOMETRY for a, b in zip(_geometry(n)[1], _geometry(n)[1][1:])} == {4, 16, 64}
    offs = [o for o, _ in _geometry("r34_ratios_4_16_64")[0]]
    assert offs != sorted(offs)
    seqs, reds = _geometry("one_long_sequence")
    n_sec = sum((n + 1023) // 1024 for _, n in seqs)
    n0 = sum((n + reds[0] - 1) // reds[0] for _, n in seqs)
    assert n0 > 3 * 1024 and n0 % 1024 and n_sec + (n0 + 1023) // 1024 > 1024
    assert len(_geometry("many_short_sequences")[0]) > 2000 and not _geometry("no_sequence")[0]


def _start_rc(engine, uniq, off, ln, reds):
    L = eng.load()
    off, ln, reds = np.asarray(off, np.uint64), np.asarray(ln, np.uint32), np.asarray(reds, np.uint32)
    h = C.c_void_p()
    rc = L.itx_bigwig_start(engine._h, uniq, eng._p(off), eng._p(ln), len(ln), eng._p(reds), len(reds), C.byref(h))
    msg = L.itx_last_error().decode(errors="replace")
    if h.value:
        L.itx_bigwig_destroy(h)
    return rc, msg


def test_argument_checks(rig):
    """ordinary error returns, before anything is launched"""
    rig.load("small")
    e = rig.engine
    bad = {
        "a length of 0": ([0, 10], [5, 0], [10, 40]),
        "a window past the coverage": ([COV_LEN - 5], [10], [10, 40]),
        "an offset past the coverage": ([COV_LEN + 1], [1], [10]),
        "offset + length wraps around 2^64": ([2 ** 64 - 1], [2], [10]),
        "a ratio of 3": ([0], [100], [10, 30]),
        "a ratio of 1.5": ([0], [100], [10, 15]),
        "a ratio of 1": ([0], [100], [10, 10]),
        "a ratio of 8": ([0], [100], [10, 80]),
        "a ratio of 2 after one of 4": ([0], [100], [10, 40, 80]),
        "a falling reduction": ([0], [100], [40, 10]),
        "a reduction of 0": ([0], [100], [0]),
        "11 levels": ([0], [100], [4 ** k for k in range(11)]),
    }
    for what, (off, ln, reds) in bad.items():
        rc, msg = _start_rc(e, 0, off, ln, reds)
        assert rc == E_ARG and msg, f"{what}: rc {rc}, message {msg!r}"
    # and neighbours of those that are fine
    for off, ln, reds in (([COV_LEN - 10], [10], [10, 40]), ([0], [COV_LEN], [34]), ([0], [100], [10, 160])):
        rc, msg = _start_rc(e, 1, off, ln, reds)
        assert rc == 0, msg


def test_state_checks(rig):
    fresh = eng.Engine(rig.table, {}, batch_capacity=1 << 12)
    rc, msg = _start_rc(fresh, 0, [0], [100], [10])
    assert rc == E_STATE and msg, (rc, msg)
    fresh.close()
    flt = eng.Engine(rig.table, {"filter_mode": True}, batch_capacity=1 << 12)
    flt.set_tidmap([0])
    rc, msg = _start_rc(flt, 0, [0], [100], [10])
    assert rc == E_STATE and msg, (rc, msg)
    flt.finish()
    rc, msg = _start_rc(flt, 0, [0], [100], [10])
    assert rc == E_STATE and msg, (rc, msg)
    flt.close()
