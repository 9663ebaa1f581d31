"""GPU: the bed files of `stat -B / -V` built on the device (include/iteres_amd.h itx_bed_*, csrc/itx_bed.hip).
1. the ABI, directly: windows of raw BAM records with awkward names and tags (tests/bedcase.py) through the inflater's parse and
   itx_bamwin_bed, both texts byte for byte against Python's own formatting of an independent reading;
2. the command three ways (device route, ITX_HOST_BED=1, the reference binary where it is built), files compared whole;
3. files whose batches alternate between the two routes; 4. the committed golden runs; 5. one run at size."""
import ctypes as C
import filecmp
import hashlib
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import bedcase as bc
import goldencase as gc
import refio
from iteres_amd import build, engine as eng, synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.path.join(ROOT, "oracle", "_ref", "iteres")
HEADER = [("chr1", 2147483647), ("MT", 16571), ("GL000191.1", 106433), ("1", 2147483647)]
TILE = 256                                   # records per workgroup of k_bed_write (csrc/itx_bed.hip BED_TILE)


# ---- 1. the ABI

def window(inf, comp):
    """the whole file into window 0, header skipped, records parsed -> number of records"""
    L = eng.load()
    blocks = eng.index_bgzf(comp)
    cbuf = np.zeros(len(comp) + 16, np.uint8)
    cbuf[:len(comp)] = np.frombuffer(comp, np.uint8)
    status = np.full(len(blocks), 255, np.uint8)
    n_new = C.c_size_t()
    eng._chk(L.itx_bamwin_push(inf._h, 0, eng._p(cbuf), len(comp), eng._p(blocks), len(blocks), eng._p(status), C.byref(n_new)), "push")
    assert (status == 0).all()
    raw = np.zeros(min(n_new.value, 1 << 16), np.uint8)
    eng._chk(L.itx_bamwin_peek(inf._h, 0, 0, eng._p(raw), len(raw)), "peek")
    b = raw.tobytes()
    l_text, = struct.unpack_from("<i", b, 4)
    p = 8 + l_text
    n_ref, = struct.unpack_from("<i", b, p)
    p += 4
    for _ in range(n_ref):
        l_name, = struct.unpack_from("<i", b, p)
        p += 4 + l_name + 4
    eng._chk(L.itx_bamwin_skip(inf._h, 0, p), "skip")
    n_rec, mal, fl, redo = C.c_size_t(), C.c_int(), C.c_int(), C.c_size_t()
    eng._chk(L.itx_bamwin_parse(inf._h, 0, n_ref, C.byref(n_rec), C.byref(mal), C.byref(fl), C.byref(redo)), "parse")
    return n_rec.value


def fetch(inf, n):
    arrs = {"tid": np.zeros(n, np.int32), "pos": np.zeros(n, np.int32), "tmpend": np.zeros(n, np.int32), "mapq": np.zeros(n, np.uint8),
            "flag5": np.zeros(n, np.uint8), "mpos": np.zeros(n, np.int32), "isize": np.zeros(n, np.int32)}
    st = eng.Staging(*[arrs[k].ctypes.data for k in ("tid", "pos", "tmpend", "mapq", "flag5", "mpos", "isize")], None, n)
    off = np.zeros(n, np.uint32)
    eng._chk(eng.load().itx_bamwin_fetch(inf._h, 0, n, C.byref(st), 0, eng._p(off), None), "fetch")
    return arrs, off


def bulk_records(seed, n):
    """ordinary reads with XA strings of every length up to a few hundred bytes: lines that cross every kind of 16-byte and
    window boundary"""
    rng = np.random.default_rng(seed)
    R = []
    for i in range(n):
        fl = int(rng.choice([0, 16, 0x1 | 0x40, 0x1 | 0x40 | 0x10, 0x1 | 0x80, 4]))
        aux = b""
        if rng.random() < 0.4:
            aux = bc.tag("NM", "C", bytes([int(rng.integers(0, 9))])) + bc.tag("XA", "Z", b"chr%d,+%d,36M,1;" % (i % 23, i) * int(rng.integers(0, 12)) + b"\0")
        pos = int(rng.integers(0, 10 ** int(rng.integers(1, 10))))
        isz = int(rng.choice([0, 180, -180, 320, -320, 900]))
        R.append(bc.record(tid=int(rng.integers(0, 4)), pos=pos, mapq=int(rng.choice([0, 3, 9, 10, 30, 37, 60])), flag=fl, qname=b"read.%d/%d\0" % (seed, i),
                           cigar=((0, int(rng.integers(20, 150))),), mtid=0, mpos=max(pos - 100, 0), isize=isz, aux=aux))
    return R


def device_texts(inf, recs, p, add_chr=False, want=3, batches=None, dedup=False, cap=1 << 16):
    """both texts of the records through the window route, batch after batch; and the expectation"""
    n = window(inf, bc.bam_bytes(HEADER, recs))
    assert n == len(recs)
    names = [gc.rename_chr(nm, add_chr) for nm, _ in HEADER]
    chrom_names = [c for c in dict.fromkeys(names) if c is not None]
    sizes = [next(l for (h, l), nm in zip(HEADER, names) if nm == c) for c in chrom_names]
    skip = None
    t2c = [(-2 if nm is None else chrom_names.index(nm)) for nm in names]
    if dedup:
        dd = eng.Dedup(sizes, p)
        dd.set_tidmap(t2c, [0 if nm is None else chrom_names.index(nm) for nm in names])
        eng._chk(eng.load().itx_bamwin_dedup(inf._h, dd._h), "itx_bamwin_dedup")
        skip = (fetch(inf, n)[0]["flag5"] & eng.F5_NOLOOKUP) != 0
        dd.close()
    want_b, want_v, t2c_py, _ = bc.lines(p, HEADER, chrom_names, sizes, recs, add_chr, skip)
    assert t2c_py == t2c
    bed = eng.Bed(sizes, p, want=want, batch_capacity=cap)
    bed.set_tidmap(t2c, names)
    got_b, got_v = [], []
    first = 0
    for m in (batches or [n]):
        assert bed.start_window(inf, first, m) == 0
        b, v = bed.collect()
        got_b.append(b)
        got_v.append(v)
        first += m
    assert first == n
    st = bed.stats()
    bed.close()
    return b"".join(got_b), b"".join(got_v), (want_b if want & 1 else b""), (want_v if want & 2 else b""), skip, st


@pytest.fixture(scope="module")
def inf():
    h = eng.Inflater()
    yield h
    h.close()


OPTS = [("default", {}, False), ("E0", dict(extension=0), False), ("T", dict(treat_pe_as_se=True), False), ("D", dict(discard_half_mapped=True), False),
        ("I", dict(isize_max=200), False), ("Q0", dict(mapq_min=0), False), ("Q30", dict(mapq_min=30), False), ("C", {}, True)]


@pytest.mark.parametrize("name,opt,add_chr", OPTS, ids=[o[0] for o in OPTS])
def test_window_texts_equal_python_formatting(inf, name, opt, add_chr):
    recs = bc.corner_records() + bulk_records(5, 3000)
    got_b, got_v, want_b, want_v, _, st = device_texts(inf, recs, bc.params(**opt), add_chr)
    assert got_b == want_b
    assert got_v == want_v
    assert want_b.count(b"\n") > 1000 and 0 < want_v.count(b"\n") <= want_b.count(b"\n")
    assert st["batches"] == 1 and st["bytes"] == len(want_b) + len(want_v) and st["kernel_ms"] > 0


@pytest.mark.parametrize("want", [eng.BED_ALL, eng.BED_UNIQ], ids=["B-alone", "V-alone"])
def test_one_file_alone(inf, want):
    recs = bc.corner_records() + bulk_records(6, 1000)
    got_b, got_v, want_b, want_v, _, _ = device_texts(inf, recs, bc.params(), want=want)
    assert got_b == want_b and got_v == want_v
    assert (len(got_b) > 0) == (want == eng.BED_ALL) and (len(got_v) > 0) == (want == eng.BED_UNIQ)


@pytest.mark.parametrize("paired", [False, True], ids=["single", "paired"])
def test_records_marked_by_the_device_dedup_have_no_line(inf, paired):
    one = [bc.record(tid=0, pos=5000 + (i // 7), mapq=[37, 3][i % 5 == 4], flag=(0x1 | 0x40 if paired else 0) | (16 if i % 3 == 0 else 0), qname=b"d%d\0" % i,
                     mtid=0, mpos=5100, isize=200 if paired else 0, aux=bc.tag("XA", "Z", b"x,+1,2M,0;\0") if i % 2 else b"") for i in range(2000)]
    got_b, got_v, want_b, want_v, skip, _ = device_texts(inf, one, bc.params(), dedup=True)
    assert skip.sum() > 500 and not skip.all()
    assert got_b == want_b and got_v == want_v


def test_geometries(inf):
    p = bc.params(extension=0)
    # a batch of one record
    got_b, got_v, want_b, want_v, _, _ = device_texts(inf, [bc.record(pos=41, qname=b"only\0")], p)
    assert (got_b, got_v) == (want_b, want_v) and got_b == b"chr1\t41\t91\tonly\t37\t+\n"
    # no record has a line: both sizes 0
    got_b, got_v, want_b, want_v, _, st = device_texts(inf, [bc.record(flag=4, qname=b"u%d\0" % i) for i in range(700)], p)
    assert got_b == got_v == want_b == want_v == b"" and st["bytes"] == 0
    # a window holding several batches; `first` not at 0, not at a tile's start
    recs = bulk_records(9, 5000)
    got_b, got_v, want_b, want_v, _, st = device_texts(inf, recs, p, batches=[16, 1, 999, 2048, 1936], cap=2048)
    assert got_b == want_b and got_v == want_v and st["batches"] == 5
    # long XA strings around a tile's end: the tile's last record, the next tile's first one, and one that spans several windows of LDS
    long1, long2, long3 = (bc.tag("XA", "Z", bytes([65 + k]) * ln + b"\0") for k, ln in enumerate((40_000, 33_000, 150_000)))
    recs = bulk_records(10, TILE - 1) + [bc.record(pos=1, qname=b"last-of-tile\0", aux=long1), bc.record(pos=2, qname=b"first-of-tile\0", aux=long2)] + bulk_records(11, 300) + \
        [bc.record(pos=3, qname=b"mid\0", aux=long3)] + bulk_records(12, 100)
    got_b, got_v, want_b, want_v, _, _ = device_texts(inf, recs, p)
    assert got_b == want_b and got_v == want_v
    assert b"A" * 40_000 + b"\n" in got_b and b"C" * 150_000 + b"\n" in got_b
    # one batch of 1026 tiles: every thread of the tile scan's workgroup (1024) takes two tiles, the last chunk ragged, the rest empty
    n = 1024 * TILE + 257
    recs = [bc.record(tid=i % 4, pos=100 + i, mapq=[37, 3][i % 5 == 4], flag=16 if i % 3 == 0 else 0, qname=b"t%d\0" % i, cigar=((0, 20),)) for i in range(n)]
    got_b, got_v, want_b, want_v, _, st = device_texts(inf, recs, p, cap=n)
    assert got_b == want_b and got_v == want_v and st["batches"] == 1
    assert want_b.count(b"\n") > 1025 * TILE > want_v.count(b"\n") > 0


def test_lifecycle_and_slot_outputs_that_regrow(inf):
    """made and destroyed with no call between; then, twice in one process: made, a batch of one record into either slot, then a batch
    of 1000 into either slot, so that all four outputs of both slots (device and page-locked, -B and -V) are dropped and taken anew
    under one object, both texts byte for byte the expectation's; destroyed"""
    eng.Bed([1000], batch_capacity=16).close()
    p = bc.params(extension=0)
    recs = [bc.record(pos=41, qname=b"only\0"), bc.record(pos=42, qname=b"next\0")] + bulk_records(13, 2000)
    for _ in range(2):
        got_b, got_v, want_b, want_v, _, st = device_texts(inf, recs, p, batches=[1, 1, 1000, 1000], cap=1000)
        assert got_b == want_b and got_v == want_v and st["batches"] == 4
        assert got_b.startswith(b"chr1\t41\t91\tonly\t37\t+\nchr1\t42\t92\tnext\t37\t+\n") and got_v.startswith(b"chr1\t41\t91\tonly\t37\t+\n")
    # a batch of one line (23 bytes) leaves room for need + need / 4 + 4096 bytes: either text of either large batch is beyond it
    names, sizes = [nm for nm, _ in HEADER], [l for _, l in HEADER]
    for lo in (2, 1002):
        assert min(len(t) for t in bc.lines(p, HEADER, names, sizes, recs[lo:lo + 1000])[:2]) > 23 + 23 // 4 + 4096


def test_plain_device_arrays_and_two_batches_in_flight(inf):
    """itx_bed_run over torch tensors gives the window route's text; two batches may be started before the first is collected, and
    come back oldest first"""
    import torch
    p = bc.params()
    recs = bc.corner_records() + bulk_records(7, 1500)
    _, _, want_b, want_v, _, _ = device_texts(inf, recs, p)
    arrs, _ = fetch(inf, len(recs))
    off = np.cumsum([0] + [len(r) for r in recs[:-1]]).astype(np.int64)
    dev = torch.device("cuda:0")
    t = {k: torch.from_numpy(v).to(dev) for k, v in arrs.items()}
    raw = torch.from_numpy(np.frombuffer(b"".join(recs) + bytes(64), np.uint8).copy()).to(dev)
    roff = torch.from_numpy(off.astype(np.uint32).view(np.int32)).to(dev)
    names = [nm for nm, _ in HEADER]
    bed = eng.Bed([l for _, l in HEADER], p, batch_capacity=len(recs))
    bed.set_tidmap([0, 1, 2, 3], names)
    k = 700
    half = lambda a, lo, hi: {n: v[lo:hi].contiguous() for n, v in a.items()}
    a, b = half(t, 0, k), half(t, k, len(recs))
    assert bed.run(raw, roff[:k].contiguous(), a["tid"], a["pos"], a["tmpend"], a["mapq"], a["flag5"], a["mpos"], a["isize"]) == 0
    assert bed.run(raw, roff[k:].contiguous(), b["tid"], b["pos"], b["tmpend"], b["mapq"], b["flag5"], b["mpos"], b["isize"]) == 0
    with pytest.raises(eng.ItxError):                                   # a third one has no slot
        bed.run(raw, roff[:k].contiguous(), a["tid"], a["pos"], a["tmpend"], a["mapq"], a["flag5"], a["mpos"], a["isize"])
    with pytest.raises(eng.ItxError):                                   # nor may the names change under a started batch
        bed.set_tidmap([0, 1, 2, 3], names)
    b1, v1 = bed.collect()
    b2, v2 = bed.collect()
    assert b1 + b2 == want_b and v1 + v2 == want_v
    with pytest.raises(eng.ItxError):
        bed.collect()                                                   # nothing is started
    # a name that runs out of its record: the host has to look, nothing is started
    odd = bc.record(qname=b"abc", cigar=(), l_qseq=0)
    raw2 = torch.from_numpy(np.frombuffer(odd + bytes(64), np.uint8).copy()).to(dev)
    z = torch.zeros(1, dtype=torch.int32, device=dev)
    assert bed.run(raw2, z, z, z + 5, z + 9, torch.full((1,), 40, dtype=torch.uint8, device=dev), torch.zeros(1, dtype=torch.uint8, device=dev)) == 1
    with pytest.raises(eng.ItxError):
        bed.collect()
    bed.close()


def test_argument_checks():
    L = eng.load()
    h = C.c_void_p()
    cs = np.array([1000], np.int64)
    p = eng.Params(10, 1e-4, 150, 500, 0, 0, 0, 0)
    assert L.itx_bed_create(0, None, 1, C.byref(p), 3, 16, C.byref(h)) == -1
    assert L.itx_bed_create(0, eng._p(cs), 1, C.byref(p), 0, 16, C.byref(h)) == -1            # neither file wanted
    assert L.itx_bed_create(0, eng._p(cs), 1, C.byref(p), 4, 16, C.byref(h)) == -1
    assert L.itx_bed_create(0, eng._p(cs), 1, C.byref(p), 3, 0, C.byref(h)) == -1
    assert L.itx_bed_collect(None, None) == -1 and L.itx_bed_get_stats(None, None) == -1 and L.itx_bed_set_tidmap(None, None, None, 0) == -1
    bed = eng.Bed(cs, batch_capacity=16)
    hard = C.c_uint64()
    b = eng.Batch()
    assert L.itx_bed_run(bed._h, None, None, C.byref(b), 0, C.byref(hard)) == -5              # ITX_E_STATE: no tid map yet
    bed.set_tidmap([0], ["chr1"])
    assert L.itx_bed_run(bed._h, None, None, C.byref(b), 17, C.byref(hard)) == -1             # records without arrays
    assert L.itx_bed_run(bed._h, None, None, None, 0, C.byref(hard)) == -1
    assert L.itx_bamwin_bed(None, bed._h, 0, 0, C.byref(hard)) == -1
    bed.close()


# ---- 2. / 3. the command

@pytest.fixture(scope="module")
def exe():
    lib, exe = build.build_all()
    return exe


def _run(exe, d, out, opts, env=None, aln="reads.bam", sizes="chrom.sizes"):
    os.makedirs(out, exist_ok=True)
    pr = subprocess.run([exe, "stat"] + list(opts) + ["-B", "-V", "-o", "out", str(d / sizes), str(d / "rep.sizes"), str(d / "rmsk.txt")] + [aln if "," in aln else str(d / aln)],
                        cwd=out, capture_output=True, text=True, timeout=900, env=dict(os.environ, ITX_TIMING="1", **(env or {})))
    assert pr.returncode == 0, pr.stderr[-2000:]
    return pr


def _same(a, b):
    names = sorted(fn for fn in os.listdir(a) if not fn.endswith(".bigWig"))
    assert len(names) == 8 and sum(fn.endswith(".bed") for fn in names) == 2, names
    for fn in names:
        assert filecmp.cmp(os.path.join(a, fn), os.path.join(b, fn), shallow=False), fn


def _bed_routes(err):
    m = re.search(r"\[itx timing\] bed: (\d+) batches built on the device \((\d+) bytes, [0-9.]+ ms in its kernels, host waited [0-9.]+ s\), (\d+) by the host", err)
    assert m, err[-1500:]
    return int(m.group(1)), int(m.group(3)), int(m.group(2))


@pytest.fixture(scope="module")
def xa_case(tmp_path_factory):
    from test_gpu_xaveto import _case
    # (the case's header has a reference the size file lacks: the windows that hold its reads are the host's, the others the device's)
    safe = _case(tmp_path_factory.mktemp("bed_xa_safe"), 810, 150_000, weird=False, ref_safe=True)
    odd = _case(tmp_path_factory.mktemp("bed_xa_odd"), 811, 40_000, weird=False, ref_safe=False)
    return safe, odd


@pytest.fixture(scope="module")
def pile_case(tmp_path_factory):
    d = tmp_path_factory.mktemp("bed_pile")
    chroms = [("chr1", 8_000_000), ("chr2", 3_000_000), ("chrM", 16_571)]
    t = synth.make_table(71, chroms, 9000, n_names=120, n_fams=14, n_clas=6, overlap_frac=0.05)
    synth.write_sizes(str(d / "chrom.sizes"), chroms)
    synth.write_sizes(str(d / "rep.sizes"), t.rep_len.items())
    synth.write_rmsk(str(d / "rmsk.txt"), t)
    mk = os.path.join(ROOT, "tools", "mkbam")
    subprocess.check_call(["gcc", "-O2", "-fopenmp", "-o", mk, os.path.join(ROOT, "tools", "mkbam.c"), "-lz", "-ldl"])
    subprocess.check_call([mk, str(d / "chrom.sizes"), "400000", str(d / "reads.bam"), "50", "11", "300", "content=hiseq", "cigar=mixed", "pileup=40"])
    return d


CMD_OPTS = [("-w",), ("-w", "-R"), ("-w", "-C"), ("-w", "-x"), ("-w", "-T", "-R", "-Q", "30")]


@pytest.mark.parametrize("opts", CMD_OPTS, ids=["".join(o) for o in CMD_OPTS])
def test_command_three_ways_xa_content(opts, xa_case, exe, tmp_path):
    env = {"ITX_BGZF_CHUNK": "3000000"}
    for k, d in enumerate(xa_case):
        env_k = dict(env, ITX_BGZF_CHUNK="300000") if k else env                  # the second file in many windows
        dev = _run(exe, d, str(tmp_path / f"dev{k}"), opts, env_k)
        host = _run(exe, d, str(tmp_path / f"host{k}"), opts, dict(env_k, ITX_HOST_BED="1"))
        _same(str(tmp_path / f"dev{k}"), str(tmp_path / f"host{k}"))
        n_dev, n_host, n_bytes = _bed_routes(dev.stderr)
        assert n_dev >= 1, (n_dev, n_host)
        assert _bed_routes(host.stderr)[0] == 0 and _bed_routes(host.stderr)[1] >= 1
    if not os.path.exists(REF):
        pytest.skip("reference binary not built")
    _run(REF, xa_case[0], str(tmp_path / "ref"), opts)
    _same(str(tmp_path / "dev0"), str(tmp_path / "ref"))


@pytest.mark.parametrize("opts", [("-w",), ("-w", "-R"), ("-w", "-R", "-E", "0")], ids=["w", "wR", "wRE0"])
def test_command_three_ways_pileup(opts, pile_case, exe, tmp_path):
    env = {"ITX_BGZF_CHUNK": "3000000"}
    dev = _run(exe, pile_case, str(tmp_path / "dev"), opts, env)
    host = _run(exe, pile_case, str(tmp_path / "host"), opts, dict(env, ITX_HOST_BED="1"))
    _same(str(tmp_path / "dev"), str(tmp_path / "host"))
    n_dev, n_host, _ = _bed_routes(dev.stderr)
    assert n_dev >= 3 and n_host == 0, (n_dev, n_host)                            # many windows, all of them on the device
    assert _bed_routes(host.stderr)[0] == 0
    if not os.path.exists(REF):
        pytest.skip("reference binary not built")
    _run(REF, pile_case, str(tmp_path / "ref"), opts)
    _same(str(tmp_path / "dev"), str(tmp_path / "ref"))


def test_mixed_routes_unknown_chromosome(pile_case, exe, tmp_path):
    """a size file that lacks one reference: the windows with reads on it go to the host (its warning is per record), the others stay
    on the device; same files as the all-host run, the warning once"""
    lines_ = open(pile_case / "chrom.sizes").read().splitlines()
    open(pile_case / "short.sizes", "w").write("\n".join(l for l in lines_ if not l.startswith("chr2\t")) + "\n")
    env = {"ITX_BGZF_CHUNK": "1000000"}
    dev = _run(exe, pile_case, str(tmp_path / "dev"), ("-w", "-R"), env, sizes="short.sizes")
    host = _run(exe, pile_case, str(tmp_path / "host"), ("-w", "-R"), dict(env, ITX_HOST_BED="1"), sizes="short.sizes")
    _same(str(tmp_path / "dev"), str(tmp_path / "host"))
    n_dev, n_host, _ = _bed_routes(dev.stderr)
    assert n_dev >= 1 and n_host >= 1, (n_dev, n_host)
    assert dev.stderr.count("read ends mapped to chromosome chr2 will be discarded") == 1


def test_mixed_routes_hard_veto(exe, tmp_path):
    """XA numbers only strtol can read: the veto sends such batches to the host after their bed text was built on the device — the
    lines reach the files exactly once"""
    from test_gpu_xaveto import _case
    d = _case(tmp_path, 820, 30_000, weird=True)
    env = {"ITX_BGZF_CHUNK": "150000"}
    dev = _run(exe, d, str(tmp_path / "dev"), ("-w",), env)
    host = _run(exe, d, str(tmp_path / "host"), ("-w",), dict(env, ITX_HOST_BED="1"))
    _same(str(tmp_path / "dev"), str(tmp_path / "host"))
    n_dev, n_host, _ = _bed_routes(dev.stderr)
    assert n_dev >= 1 and n_host >= 1, (n_dev, n_host)
    if os.path.exists(REF):
        _run(REF, d, str(tmp_path / "ref"), ("-w",))
        _same(str(tmp_path / "dev"), str(tmp_path / "ref"))


def test_two_bams_with_different_headers(xa_case, pile_case, exe, tmp_path):
    d = tmp_path / "two"
    d.mkdir()
    chroms = [("chr1", 8_000_000), ("chr10", 900_000), ("chr2", 3_000_000), ("chr1_alt", 400_000)]
    synth.write_sizes(str(d / "chrom.sizes"), chroms)
    for fn in ("rep.sizes", "rmsk.txt"):
        os.symlink(pile_case / fn, d / fn)
    aln = f"{xa_case[0] / 'reads.bam'},{pile_case / 'reads.bam'}"
    env = {"ITX_BGZF_CHUNK": "2000000"}
    dev = _run(exe, d, str(tmp_path / "dev"), ("-w", "-R"), env, aln=aln)
    host = _run(exe, d, str(tmp_path / "host"), ("-w", "-R"), dict(env, ITX_HOST_BED="1"), aln=aln)
    _same(str(tmp_path / "dev"), str(tmp_path / "host"))
    assert _bed_routes(dev.stderr)[0] >= 2


# ---- 4. the goldens

@pytest.mark.parametrize("case,run_name,device", [("sidechan", "stat_B_V", True), ("addchr", "stat_C_R_B", True), ("sidechan", "stat_R_B_V_sam", False)])
def test_golden_runs(case, run_name, device, exe, tmp_path):
    run = gc.manifest_run(case, run_name)
    src = os.path.join(gc.GOLDEN, case, "in")
    paths = [refio.materialise(src, n, str(tmp_path)) for n in ["chrom.sizes", "rep.sizes", "rmsk.txt", run["aln"]]]
    work = tmp_path / "out"
    work.mkdir()
    # (both BAMs hold reads on a reference their size file lacks; in one window the whole file would be the host's for the warning's
    # sake, so the windows are kept small: the ones without such reads stay on the device)
    pr = subprocess.run([exe, run["cmd"]] + run["opts"] + ["-o", run["prefix"]] + paths, cwd=work, capture_output=True, text=True, timeout=600,
                        env=dict(os.environ, ITX_TIMING="1", ITX_BGZF_CHUNK="30000"))
    assert pr.returncode == run["rc"], pr.stderr[-2000:]
    beds = [fn for fn in run["files"] if fn.endswith(".bed")]
    assert beds
    for fn in run["files"]:
        assert (work / fn).read_bytes() == refio.read_bytes(os.path.join(gc.GOLDEN, case, run_name, fn)), fn
    n_dev, n_host, _ = _bed_routes(pr.stderr)
    assert n_dev >= 1 if device else (n_dev == 0 and n_host >= 1), (n_dev, n_host)


# ---- 5. size

def test_at_size_device_equals_host(exe, tmp_path):
    """24 M reads of hiseq content (50 bases, XA on a quarter, mixed CIGARs): six batches of 4 Mi records, 1.6 GB of text — where a
    32-bit offset or a wrapped page-locked buffer would show. Device route against host route by SHA-256 of both bed files."""
    chroms = [("chr1", 248_000_000), ("chr2", 242_000_000), ("chrX", 156_000_000)]
    t = synth.make_table(91, chroms, 60_000, n_names=300, n_fams=25, n_clas=8, overlap_frac=0.05)
    synth.write_sizes(str(tmp_path / "chrom.sizes"), chroms)
    synth.write_sizes(str(tmp_path / "rep.sizes"), t.rep_len.items())
    synth.write_rmsk(str(tmp_path / "rmsk.txt"), t)
    mk = os.path.join(ROOT, "tools", "mkbam")
    subprocess.check_call(["gcc", "-O2", "-fopenmp", "-o", mk, os.path.join(ROOT, "tools", "mkbam.c"), "-lz", "-ldl"])
    subprocess.check_call([mk, str(tmp_path / "chrom.sizes"), "24000000", str(tmp_path / "reads.bam"), "50", "31", "250", "content=hiseq", "cigar=mixed"])

    def sha(path):
        h = hashlib.sha256()
        with open(path, "rb") as f:
            for blk in iter(lambda: f.read(1 << 24), b""):
                h.update(blk)
        return h.hexdigest(), os.path.getsize(path)

    dev = _run(exe, tmp_path, str(tmp_path / "dev"), ("-w", "-R"))
    got = {fn: sha(tmp_path / "dev" / fn) for fn in ("out.iteres.bed", "out.iteres.unique.bed")}
    n_dev, n_host, n_bytes = _bed_routes(dev.stderr)
    assert n_dev >= 6 and n_host == 0 and n_bytes == sum(v[1] for v in got.values()) > 1 << 30
    for fn in got:
        os.remove(tmp_path / "dev" / fn)
    _run(exe, tmp_path, str(tmp_path / "host"), ("-w", "-R"), {"ITX_HOST_BED": "1"})
    for fn, v in got.items():
        assert sha(tmp_path / "host" / fn) == v, fn
