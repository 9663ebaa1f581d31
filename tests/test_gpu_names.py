"""GPU: the read lists of `filter -r` built on the device (include/iteres_amd.h itx_names_*, csrc/itx_names.hip).
1. the ABI, directly: windows of raw BAM records (tests/bedcase.py) through the inflater's parse and itx_bamwin_names with the chosen
   rows given as an array; the expectation is Python's own b",".join of the names in append order, per row;
2. batches, two windows and a pool that has to grow; 3. host appends between device batches; 4. a name that runs out of its record;
5. records the device -R pass marked; 6. argument checks;
7. the command three ways (device route ITX_HOST_NAMES=0, host route ITX_HOST_NAMES=1, the reference binary where it is built), files compared whole, and the
   timing line's route counters; mixed routes; the committed golden runs; SAM text."""
import ctypes as C
import filecmp
import os
import re
import subprocess

import numpy as np
import pytest

import bedcase as bc
import goldencase as gc
import refio
from iteres_amd import build, engine as eng, synth
from test_gpu_bed import HEADER, fetch, window

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.path.join(ROOT, "oracle", "_ref", "iteres")
BIG_ROWS = (1 << 24) + 5                      # four digit passes, and every one of them decides something


@pytest.fixture(scope="module")
def inf():
    h = eng.Inflater()
    yield h
    h.close()


def expect(rows, names):
    """{row: joined list}, per-row counts — the reference's rule (generic.c:662-666 + 1729-1731) in Python"""
    lists = {}
    for r, nm in zip(rows, names):
        if r >= 0:
            lists.setdefault(int(r), []).append(nm)
    return {r: b",".join(v) for r, v in lists.items()}, {r: len(v) for r, v in lists.items()}


def qname_of(rec):
    return bc.read_record(rec)["qname"]


def make_case(kind, n):
    """(records, hit rows, n_rows) — the properties a window of n records can carry"""
    rng = np.random.default_rng(1000 + n)
    recs, rows = [], np.zeros(n, np.int32)
    n_rows = {"lengths": 50, "one_row": 7, "own_row": max(n, 1), "descending": max(n, 1), "big_rows": BIG_ROWS}[kind]
    for i in range(n):
        kw = {}
        if kind == "lengths":                                             # every length 1 .. 254, commas inside, empty names, -1 interleaved
            ln = i % 254 + 1
            body = (b"%d," % i + b"n" * 254)[:ln]
            qn = body + b"\0"
            if i % 11 == 5:
                qn = b"\0"                                               # l_qname points at an empty name
            if i % 29 == 7:
                qn, kw = b"", dict(l_qname=0)                            # no name at all
            rows[i] = -1 if i % 3 == 1 else int(rng.integers(0, 50))
        elif kind == "one_row":                                           # stability: the sequence number is the name
            qn = b"s%d\0" % i
            rows[i] = 3
        elif kind == "own_row":
            qn = b"o%d\0" % i
            rows[i] = i
        elif kind == "descending":
            qn = b"d%d,x\0" % i
            rows[i] = n - 1 - i if i % 5 else -1
        else:                                                             # "big_rows": ids >= 2^16 and >= 2^24, few enough that rows repeat
            qn = b"b%d\0" % i
            rows[i] = [5, 70_000, (1 << 24) + 4, (1 << 16), (1 << 24), 255, 256, (1 << 16) - 1, 0xABCDEF, 0x1000001][int(rng.integers(0, 10))]
            if n > 300:
                rows[i] = int(rng.integers(0, BIG_ROWS)) if i % 2 else rows[i]
        recs.append(bc.record(tid=i % 4, pos=100 + i, qname=qn, cigar=((0, 20),), **kw))
    return recs, rows, n_rows


def check(got, rows, names, n_rows):
    lists, cnt, text, n_ent = got
    want, want_cnt = expect(rows, names)
    assert n_ent == sum(want_cnt.values())
    assert set(lists) == set(want)
    for r in want:
        assert lists[r] == want[r], r
    assert int(cnt.sum()) == n_ent and all(int(cnt[r]) == c for r, c in want_cnt.items())
    assert len(cnt) == n_rows and len(text) == sum(len(v) + 1 for v in want.values())


# ---- 1. one window

COUNTS = [0, 1, 63, 64, 65, 256, 257, 70_000]
KINDS = ["lengths", "one_row", "own_row", "descending", "big_rows"]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", COUNTS)
def test_one_window(inf, n, kind):
    import torch
    recs, rows, n_rows = make_case(kind, n)
    names = [qname_of(r) for r in recs]
    nm = eng.Names(batch_capacity=max(n, 1))
    if n:
        assert window(inf, bc.bam_bytes(HEADER, recs)) == n
        hits = torch.from_numpy(rows).cuda()
        assert nm.append_window(inf, 0, n, hits) == 0
        nm.wait_kernels()
    got = nm.finish(n_rows)
    check(got, rows, names, n_rows)
    st = nm.stats()
    assert st["batches"] == (1 if n else 0) and st["entries"] == int((rows >= 0).sum()) and st["bytes"] == sum(len(x) for x, r in zip(names, rows) if r >= 0)
    if kind == "one_row" and n:
        assert got[0][3] == b",".join(b"s%d" % i for i in range(n))       # append order survived every pass
    nm.close()


def test_one_batch_of_more_than_1024_tiles(inf):
    """1026 tiles in ONE batch: the tile scan's workgroup has 1024 threads, so each takes a chunk of two tiles, walks it twice (sum,
    then write back), the last chunk is ragged and the threads behind it are empty. (finish scans the text over 684 tiles.)"""
    import torch
    n = 1024 * 256 + 257
    recs = [bc.record(tid=i % 4, pos=100 + i, qname=b"t%d\0" % i, cigar=((0, 20),)) for i in range(n)]
    names = [b"t%d" % i for i in range(n)]
    idx = np.arange(n)
    rows = np.where(idx % 3 != 1, idx % 50, -1).astype(np.int32)
    nm = eng.Names(batch_capacity=n)
    assert window(inf, bc.bam_bytes(HEADER, recs)) == n
    assert nm.append_window(inf, 0, n, torch.from_numpy(rows).cuda()) == 0
    nm.wait_kernels()
    check(nm.finish(50), rows, names, 50)
    assert nm.stats()["batches"] == 1 and nm.stats()["entries"] == int((rows >= 0).sum())
    nm.close()


# ---- 2. batches, two windows, growth

def test_batches_two_windows_and_a_growing_pool(inf, monkeypatch):
    import torch
    monkeypatch.setenv("ITX_NAMES_POOL_BYTES", "4096")
    a, rows_a, _ = make_case("lengths", 3000)
    b, rows_b, _ = make_case("descending", 1500)
    rows_b = np.where(rows_b >= 0, rows_b % 50, -1).astype(np.int32)
    small, whole = eng.Names(batch_capacity=4096), eng.Names(batch_capacity=4096, pool_bytes=1 << 22)
    for recs, rows in ((a, rows_a), (b, rows_b)):
        n = len(recs)
        assert window(inf, bc.bam_bytes(HEADER, recs)) == n
        hits = torch.from_numpy(rows).cuda()
        first = 0
        for m in (1, 255, 256, n - 512):
            assert small.append_window(inf, first, m, hits[first:first + m]) == 0
            first += m
        assert first == n
        assert whole.append_window(inf, 0, n, hits) == 0
        small.wait_kernels()
        whole.wait_kernels()
    names = [qname_of(r) for r in a + b]
    rows = np.concatenate([rows_a, rows_b])
    g_small, g_whole = small.finish(50), whole.finish(50)
    check(g_small, rows, names, 50)
    assert g_small[0] == g_whole[0] and g_small[2] == g_whole[2] and np.array_equal(g_small[1], g_whole[1])
    assert small.stats()["grows"] >= 3 and whole.stats()["grows"] == 0 and small.stats()["batches"] == 8
    small.close()
    whole.close()


# ---- 3. host appends between device batches

def test_host_appends_keep_their_place(inf):
    import torch
    recs, rows, n_rows = make_case("lengths", 900)
    names = [qname_of(r) for r in recs]
    assert window(inf, bc.bam_bytes(HEADER, recs)) == 900
    hits = torch.from_numpy(rows).cuda()
    nm = eng.Names(batch_capacity=1024, pool_bytes=2048)
    h1 = ([4, 4, 49, 0], [b"host,1", b"", b"h" * 254, b"x"])
    h2 = ([0, 4], [b"tail-a", b"tail-b"])
    nm.append_host([7], [b"first-of-all"])
    assert nm.append_window(inf, 0, 300, hits[:300]) == 0
    nm.append_host(*h1)
    nm.append_host([], [])
    assert nm.append_window(inf, 300, 600, hits[300:]) == 0
    nm.append_host(*h2)
    all_rows = [7] + list(rows[:300]) + h1[0] + list(rows[300:]) + h2[0]
    all_names = [b"first-of-all"] + names[:300] + h1[1] + names[300:] + h2[1]
    check(nm.finish(n_rows), all_rows, all_names, n_rows)
    assert nm.stats()["host_batches"] == 3 and nm.stats()["batches"] == 2
    nm.close()


# ---- 4. a name without a NUL inside its record

def test_hard_record_appends_nothing():
    import torch
    dev = torch.device("cuda:0")
    good = [bc.record(qname=b"g%d\0" % i) for i in range(300)]
    odd = bc.record(qname=b"abc", cigar=(), l_qseq=0)
    nm = eng.Names(batch_capacity=1024)

    def tensors(recs):
        off = np.cumsum([0] + [len(r) for r in recs[:-1]]).astype(np.uint32)
        raw = torch.from_numpy(np.frombuffer(b"".join(recs) + bytes(64), np.uint8).copy()).to(dev)
        return raw, torch.from_numpy(off.view(np.int32)).to(dev)
    raw, off = tensors(good)
    rows = torch.arange(300, dtype=torch.int32, device=dev) % 5
    assert nm.run(raw, off, rows) == 0
    before = nm.stats()
    mixed = good[:100] + [odd] + good[100:200]
    raw2, off2 = tensors(mixed)
    assert nm.run(raw2, off2, torch.ones(201, dtype=torch.int32, device=dev)) == 1
    after = nm.stats()
    assert after["entries"] == before["entries"] == 300 and after["bytes"] == before["bytes"] and after["hard_batches"] == 1 and after["batches"] == 1
    # the same record without a chosen row is nobody's business
    none = torch.ones(201, dtype=torch.int32, device=dev)
    none[100] = -1
    assert nm.run(raw2, off2, none) == 0
    lists, cnt, _, n_ent = nm.finish(5)
    assert n_ent == 500 and int(cnt[1]) == 60 + 200
    assert lists[0] == b",".join(b"g%d" % i for i in range(0, 300, 5))
    nm.close()


# ---- 5. records the device -R pass marked never choose a row

def test_dedup_marks_have_no_name(inf):
    import torch
    from test_gpu_dedup import CHROM_SIZE, model
    L = eng.load()
    p = dict(mapq_min=10, min_cov=1e-4, extension=150, isize_max=500, treat_pe_as_se=False, discard_half_mapped=False)
    n = 3000
    header = [("chr1", CHROM_SIZE[0]), ("chr2", CHROM_SIZE[1]), ("tiny", CHROM_SIZE[2]), ("chr4", CHROM_SIZE[3])]
    rng = np.random.default_rng(77)
    pos = (rng.integers(0, 40, n) * 1000 + rng.integers(0, 4, n)).astype(np.int32)
    recs = [bc.record(tid=int(i % 2), pos=int(pos[i]), mapq=[37, 3][i % 5 == 4], flag=16 if i % 3 == 0 else 0, qname=b"q%d\0" % i) for i in range(n)]
    assert window(inf, bc.bam_bytes(header, recs)) == n
    dd = eng.Dedup(CHROM_SIZE, p)
    dd.set_tidmap([0, 1, 2, 3], [0, 1, 2, 3])
    eng._chk(L.itx_bamwin_dedup(inf._h, dd._h), "itx_bamwin_dedup")
    dd.close()
    arrs, _ = fetch(inf, n)
    marked = (arrs["flag5"] & eng.F5_NOLOOKUP) != 0
    want_drop, _ = model(p, [0, 1, 2, 3], [0, 1, 2, 3], (arrs["tid"], arrs["pos"], arrs["tmpend"], arrs["mapq"], arrs["flag5"] & ~np.uint8(eng.F5_NOLOOKUP),
                                                             arrs["mpos"], arrs["isize"]), [set(), None])
    assert np.array_equal(marked, want_drop) and 500 < marked.sum() < n - 50
    # a table with a repeat under every read: every live mapped record chooses a row
    m = 80
    rows = eng.make_rows(np.arange(m) % 2, (np.arange(m) // 2) * 1000, (np.arange(m) // 2) * 1000 + 900, np.zeros(m), np.full(m, 100), np.zeros(m, np.int64),
                         np.zeros(m, np.int64), np.zeros(m, np.int64))
    tab = eng.Table(rows, np.array(CHROM_SIZE, np.int64), np.array([300], np.uint32), 1, 1)
    e = eng.Engine(tab, p, batch_capacity=4096)
    e.set_tidmap([0, 1, 2, 3])
    db = eng.Batch()
    eng._chk(L.itx_bamwin_device_batch(inf._h, 0, 0, C.byref(db)), "itx_bamwin_device_batch")
    hits = torch.full((n,), -7, dtype=torch.int32, device="cuda:0")
    nm = eng.Names(batch_capacity=4096)
    eng._chk(L.itx_engine_classify_device(e._h, C.byref(db), n, C.c_void_p(hits.data_ptr()), nm._stream()), "itx_engine_classify_device")
    assert nm.append_window(inf, 0, n, hits) == 0
    h = hits.cpu().numpy()
    assert (h[marked] == -1).all() and (h[~marked] >= 0).sum() > 500
    got = nm.finish(m)
    check(got, h, [b"q%d" % i for i in range(n)], m)
    joined = b"," + b",".join(got[0].values()) + b","
    assert not any(b",q%d," % i in joined for i in np.flatnonzero(marked)[:200])
    nm.close()
    e.close()
    tab.close()


# ---- 6. argument checks

def test_argument_checks(inf):
    import torch
    L = eng.load()
    h = C.c_void_p()
    hard = C.c_uint64()
    res = eng.NamesResult()
    assert L.itx_names_create(0, 0, 0, C.byref(h)) == -1 and L.itx_names_create(0, 16, 0, None) == -1
    assert L.itx_names_finish(None, 1, C.byref(res)) == -1 and L.itx_names_get_stats(None, None) == -1 and L.itx_names_wait_kernels(None) == -1
    assert L.itx_names_append_host(None, None, None, None, 0) == -1
    assert L.itx_names_run(None, None, None, None, 0, None, C.byref(hard)) == -1
    nm = eng.Names(batch_capacity=16)
    z = torch.zeros(64, dtype=torch.int32, device="cuda:0")
    assert L.itx_bamwin_names(None, nm._h, 0, 0, C.c_void_p(z.data_ptr()), None, C.byref(hard)) == -1
    assert L.itx_bamwin_names(inf._h, None, 0, 0, C.c_void_p(z.data_ptr()), None, C.byref(hard)) == -1
    assert L.itx_names_run(nm._h, C.c_void_p(z.data_ptr()), C.c_void_p(z.data_ptr()), C.c_void_p(z.data_ptr()), 17, None, C.byref(hard)) == -1      # above the capacity
    assert L.itx_names_run(nm._h, None, None, None, 5, None, C.byref(hard)) == -1                                                                     # records without arrays
    assert L.itx_names_run(nm._h, C.c_void_p(z.data_ptr()), C.c_void_p(z.data_ptr()), C.c_void_p(z.data_ptr()), 1, None, None) == -1
    assert L.itx_names_append_host(nm._h, None, None, None, 3) == -1
    assert L.itx_names_finish(nm._h, 0, C.byref(res)) == -1 and L.itx_names_finish(nm._h, 4, None) == -1
    nm.append_host([9], [b"beyond"])
    assert L.itx_names_finish(nm._h, 4, C.byref(res)) == -1 and b"n_rows" in L.itx_last_error()      # a row the caller's table does not have
    assert L.itx_names_finish(nm._h, 10, C.byref(res)) == 0 and res.n_entries == 1
    assert L.itx_names_finish(nm._h, 10, C.byref(res)) == -5                                          # ITX_E_STATE: called twice
    with pytest.raises(eng.ItxError):
        nm.append_host([1], [b"late"])
    nm.close()


# ---- 7. the command

@pytest.fixture(scope="module")
def exe():
    lib, exe = build.build_all()
    return exe


@pytest.fixture(scope="module")
def pile(tmp_path_factory):
    d = tmp_path_factory.mktemp("names_pile")
    chroms = [("chr1", 8_000_000), ("chr2", 3_000_000), ("chrM", 16_571)]
    t = synth.make_table(71, chroms, 9000, n_names=120, n_fams=14, n_clas=6, overlap_frac=0.05)
    synth.write_sizes(str(d / "chrom.sizes"), chroms)
    synth.write_sizes(str(d / "rep.sizes"), t.rep_len.items())
    synth.write_rmsk(str(d / "rmsk.txt"), t)
    mk = os.path.join(ROOT, "tools", "mkbam")
    subprocess.check_call(["gcc", "-O2", "-fopenmp", "-o", mk, os.path.join(ROOT, "tools", "mkbam.c"), "-lz", "-ldl"])
    subprocess.check_call([mk, str(d / "chrom.sizes"), "400000", str(d / "reads.bam"), "50", "11", "300", "content=hiseq", "cigar=mixed", "pileup=40"])
    subprocess.check_call([mk, str(d / "chrom.sizes"), "60000", str(d / "other.bam"), "50", "12", "0", "content=novaseq", "cigar=mixed"])
    big = t.clas[int(np.bincount(np.asarray(t.cla_of_row)).argmax())]
    name = t.names[int(np.bincount(np.asarray(t.rep_name)).argmax())]
    return d, big, name


def _run(exe, d, out, opts, env=None, aln="reads.bam", sizes="chrom.sizes", rc=0):
    os.makedirs(out, exist_ok=True)
    pr = subprocess.run([exe, "filter"] + list(opts) + ["-o", "out", str(d / sizes), str(d / "rep.sizes"), str(d / "rmsk.txt")] + [aln if "," in aln else str(d / aln)],
                        cwd=out, capture_output=True, text=True, timeout=600, env=dict(os.environ, ITX_TIMING="1", **(env or {})))
    assert pr.returncode == rc, pr.stderr[-2000:]
    return pr


def _same(a, b, n_files=2):
    names = sorted(os.listdir(a))
    assert len(names) == n_files and names == sorted(os.listdir(b)), (names, os.listdir(b))
    for fn in names:
        assert filecmp.cmp(os.path.join(a, fn), os.path.join(b, fn), shallow=False), fn


def _routes(err):
    m = re.search(r"\[itx timing\] names: (\d+) batches gathered on the device \((\d+) names, (\d+) bytes, [0-9.]+ ms in the gather kernels, [0-9.]+ ms sort \+ text\), (\d+) batches by the host", err)
    assert m, err[-1500:]
    return int(m.group(1)), int(m.group(4)), int(m.group(2))


OPTSETS = ["r", "rR", "rc_t3", "rT", "rC", "rn"]


@pytest.mark.parametrize("which", OPTSETS)
def test_command_three_ways(which, pile, exe, tmp_path):
    d, big, name = pile
    opts = {"r": ("-r",), "rR": ("-r", "-R"), "rc_t3": ("-r", "-c", big, "-t", "3"), "rT": ("-r", "-T"), "rC": ("-r", "-C"), "rn": ("-r", "-n", name)}[which]
    env = {"ITX_BGZF_CHUNK": "3000000", "ITX_HOST_NAMES": "0"}
    dev = _run(exe, d, str(tmp_path / "dev"), opts, env)
    host = _run(exe, d, str(tmp_path / "host"), opts, dict(env, ITX_HOST_NAMES="1"))
    _same(str(tmp_path / "dev"), str(tmp_path / "host"))
    n_dev, n_host, n_names = _routes(dev.stderr)
    assert n_dev >= 3 and n_host == 0 and n_names > 1000, (n_dev, n_host, n_names)             # many windows, all of them on the device
    assert _routes(host.stderr)[0] == 0 and _routes(host.stderr)[1] >= 3
    loci = [fn for fn in os.listdir(tmp_path / "dev") if fn.endswith(".loci")][0]
    assert sum(ln.count(",") + 1 for ln in open(tmp_path / "dev" / loci) if ln.rstrip("\n").split("\t")[-1]) > 1000
    if os.path.exists(REF):
        _run(REF, d, str(tmp_path / "ref"), opts)
        _same(str(tmp_path / "dev"), str(tmp_path / "ref"))


def test_command_two_file_list(pile, exe, tmp_path):
    """`filter` opens ONE alignment file (generic.c:363-373; only `stat` chops its argument at commas, generic.c:725): a list of two
    BAMs whose headers differ is the name of a file that does not exist, for the reference and for both routes here alike. What is
    compared is therefore that end — same exit status, no output file, the same complaint — on the device route, with
    ITX_HOST_NAMES=1 and, where it is built, with the reference. (Lists in file order over several windows with different headers:
    test_batches_two_windows_and_a_growing_pool.)"""
    d, _, _ = pile
    aln = f"{d / 'reads.bam'},{d / 'other.bam'}"
    runs = []
    for what, env in (("dev", {"ITX_HOST_NAMES": "0"}), ("host", {"ITX_HOST_NAMES": "1"})):
        pr = subprocess.run([exe, "filter", "-r", "-o", "out", str(d / "chrom.sizes"), str(d / "rep.sizes"), str(d / "rmsk.txt"), aln], cwd=tmp_path,
                            capture_output=True, text=True, timeout=600, env=dict(os.environ, **env))
        runs.append((pr.returncode, "Fail to open BAM file" in pr.stderr, sorted(os.listdir(tmp_path))))
    assert runs[0] == runs[1] and runs[0][0] != 0 and runs[0][1] and runs[0][2] == []
    if os.path.exists(REF):
        pr = subprocess.run([REF, "filter", "-r", "-o", "out", str(d / "chrom.sizes"), str(d / "rep.sizes"), str(d / "rmsk.txt"), aln], cwd=tmp_path,
                            capture_output=True, text=True, timeout=600)
        assert pr.returncode != 0 and "Fail to open BAM file" in pr.stderr
        assert not [fn for fn in os.listdir(tmp_path) if fn.endswith(".loci")]


def test_mixed_routes_unknown_chromosome(pile, exe, tmp_path):
    """a size file that lacks one reference: the windows with reads on it go to the host (its warning is per record), the others stay
    on the device; one ordered list all the same — the files of the all-host run, the warning once"""
    d, _, _ = pile
    lines_ = open(d / "chrom.sizes").read().splitlines()
    open(d / "short.sizes", "w").write("\n".join(l for l in lines_ if not l.startswith("chr2\t")) + "\n")
    env = {"ITX_BGZF_CHUNK": "1000000", "ITX_HOST_NAMES": "0"}
    for k, opts in enumerate((("-r",), ("-r", "-R"))):
        dev = _run(exe, d, str(tmp_path / f"dev{k}"), opts, env, sizes="short.sizes")
        host = _run(exe, d, str(tmp_path / f"host{k}"), opts, dict(env, ITX_HOST_NAMES="1"), sizes="short.sizes")
        _same(str(tmp_path / f"dev{k}"), str(tmp_path / f"host{k}"))
        n_dev, n_host, _ = _routes(dev.stderr)
        assert n_dev >= 1 and n_host >= 1, (n_dev, n_host)
        assert dev.stderr.count("read ends mapped to chromosome chr2 will be discarded") == 1


# device: whether any window can stay on the device. The `quirks` BAM is ONE BGZF block of 31 reads, two of them mapped to chrQ, which
# its size file lacks, and one to chrS, whose listed size of 2 reads as "not found" (generic.c:796-797): its only window is the
# host's, because the warning is per record in file order. The names object exists all the same and takes the host's hits
# (itx_names_append_host), and the end of the stream is the device's sort. The other BAMs are hundreds of kilobytes: many windows.
GOLDENS = [("quirks", "filter_all_r", False), ("quirks", "filter_n_AluY", False), ("mid", "filter_n", True), ("sidechan", "filter_R", True),
           ("addchr", "filter_C", True)]


@pytest.mark.parametrize("case,run_name,device", GOLDENS, ids=[g[1] for g in GOLDENS])
def test_golden_runs(case, run_name, device, exe, tmp_path):
    run = gc.manifest_run(case, run_name)
    assert "-r" in run["opts"]
    src = os.path.join(gc.GOLDEN, case, "in")
    paths = [refio.materialise(src, n, str(tmp_path)) for n in ["chrom.sizes", "rep.sizes", "rmsk.txt", run["aln"]]]
    work = tmp_path / "out"
    work.mkdir()
    # (small windows: the ones without reads on a reference the size file lacks stay on the device)
    pr = subprocess.run([exe, run["cmd"]] + run["opts"] + ["-o", run["prefix"]] + paths, cwd=work, capture_output=True, text=True, timeout=600,
                        env=dict(os.environ, ITX_TIMING="1", ITX_BGZF_CHUNK="30000", ITX_HOST_NAMES="0"))
    assert pr.returncode == run["rc"], pr.stderr[-2000:]
    for fn in run["files"]:
        assert (work / fn).read_bytes() == refio.read_bytes(os.path.join(gc.GOLDEN, case, run_name, fn)), fn
    n_dev, n_host, n_names = _routes(pr.stderr)
    print(case, run_name, "device batches", n_dev, "host batches", n_host, "names", n_names)
    assert n_names >= 1                                                  # the lists went through the device's pool and sort either way
    if device:
        assert n_dev >= 1, (n_dev, n_host)
    else:
        assert n_dev == 0 and n_host >= 1, (n_dev, n_host)
        assert "chrQ will be discarded as chrQ not existed in the chromosome size file" in pr.stderr


def test_sam_input_stays_on_the_host(exe, tmp_path):
    run = gc.manifest_run("addchr", "filter_C")
    src = os.path.join(gc.GOLDEN, "addchr", "in")
    paths = [refio.materialise(src, n, str(tmp_path)) for n in ["chrom.sizes", "rep.sizes", "rmsk.txt", "reads.sam"]]
    outs = []
    for what, env in (("dev", {"ITX_HOST_NAMES": "0"}), ("host", {"ITX_HOST_NAMES": "1"})):
        work = tmp_path / what
        work.mkdir()
        pr = subprocess.run([exe, "filter", "-S"] + run["opts"] + ["-o", run["prefix"]] + paths, cwd=work, capture_output=True, text=True, timeout=600,
                            env=dict(os.environ, ITX_TIMING="1", **env))
        assert pr.returncode == 0, pr.stderr[-2000:]
        n_dev, n_host, _ = _routes(pr.stderr)
        assert n_dev == 0 and n_host >= 1
        outs.append(str(work))
    _same(outs[0], outs[1], n_files=len(os.listdir(outs[0])))
    assert any(fn.endswith(".loci") and os.path.getsize(os.path.join(outs[0], fn)) > 0 for fn in os.listdir(outs[0]))
