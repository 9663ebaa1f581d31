"""GPU: SAM text split and parsed on the device (include/iteres_amd.h itx_samtext_*, csrc/itx_samtext.hip; the line rule:
csrc/itx_samline.h).
1. the ABI on built chunks, field by field against the host reader's own parser (iteres_amd/host/test/reader_dump) on the same
   bytes, the strings cut out of the text by the offsets that come back;
2. the command: every SAM golden under ITX_HOST_SAM=0 with small and large chunks, byte-identical to the stored files and to
   ITX_HOST_SAM=1; a reference name the header lacks in mid-file; a random draw through the reference binary where it is built."""
import ctypes as C
import filecmp
import os
import re
import subprocess

import numpy as np
import pytest

import goldencase as gc
import hosttool
import refio
from iteres_amd import build, engine as eng, synth
from test_samline import HEADER, XA1, expect_aux, make_line, named_cases, pick_plain

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.path.join(ROOT, "oracle", "_ref", "iteres")
NAMES = [b"chr1", b"chr2", b"chrX", b"chr2"]           # HEADER's @SQ lines: the second chr2 never wins a lookup
TILE, WIN = 16384, 24576                                # bytes per tile of the line search; LDS bytes a wave stages its 64 lines in
MAX_CHUNK = 8 << 20


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("bin") / "reader_dump")
    return hosttool.build(exe, "reader_dump.c")


@pytest.fixture(scope="module")
def sam():
    x = eng.SamText(NAMES, MAX_CHUNK)
    yield x
    x.close()


def host_records(dump, body: bytes, d, header=HEADER):
    path = os.path.join(str(d), "chunk.sam")
    with open(path, "wb") as f:
        f.write(header.encode() + body)
    env = {k: v for k, v in os.environ.items() if k not in ("ITX_SAM_CHUNK", "ITX_HOST_SAM")}
    pr = subprocess.run([dump, path, "1", "65536"], capture_output=True, env=env)
    assert pr.returncode == 0, pr.stderr
    assert not pr.stderr, pr.stderr[:400]               # a plain chunk makes the host parser say nothing
    out = pr.stdout.decode("latin-1").split("\n")
    return [l.split("\t") for l in out if l and l[0] not in "@#"], [l for l in out if l.startswith("#")][0]


def line(i, seq_len=36, opt=(), flag="0", eol="\n", pos=None):
    """a plain line; its length grows byte for byte with seq_len (SEQ and QUAL both)"""
    f = [f"q{i}", flag, "chr1" if i % 3 else "chr2", str(1000 + i if pos is None else pos), "37", f"{seq_len}M", "=", str(2000 + i), str(-i), "A" * seq_len,
         "I" * seq_len] + list(opt)
    return ("\t".join(f) + eol).encode()


def check_chunk(sam, dump, d, text: bytes, final=True, slot=0, expect_lines=None):
    """parses text on the device and holds every record against the host reader on the consumed bytes"""
    res = sam.parse(text, final, slot)
    assert res["n_hard"] == 0, res
    used = text[: res["consumed"]]
    if final:
        assert res["consumed"] == len(text)
    else:
        assert res["consumed"] == text.rfind(b"\n") + 1
    recs, tail = host_records(dump, used, d)
    assert res["n_lines"] == res["n_rec"] == len(recs)
    if expect_lines is not None:
        assert res["n_lines"] == expect_lines
    n = len(recs)
    a = sam.fetch(slot, 0, n)
    host = np.array([[int(x) for x in r[:7]] for r in recs], np.int64).reshape(n, 7)
    for k, name in enumerate(("tid", "pos", "tmpend", "mapq", "flag5", "mpos", "isize")):
        bad = np.flatnonzero(a[name].astype(np.int64) != host[:, k])
        assert bad.size == 0, (name, int(bad[0]), int(a[name][bad[0]]), recs[bad[0]])
    starts = [0] + [m.end() for m in re.finditer(b"\n", used)]
    any_xa = False
    for i in range(n):
        lo = int(a["line_off"][i])
        assert lo == starts[i]
        assert used[lo:lo + int(a["qname_len"][i])].decode("latin-1") == recs[i][7], i
        stop = used.find(b"\n", lo)
        has_xa, nm, xa = expect_aux(used[lo: stop if stop >= 0 else len(used)].decode("latin-1"))
        assert int(a["xa_mark"][i] != 0) == has_xa, i
        if has_xa:
            any_xa = True
            xo = int(a["xa_off"][i])
            assert used[xo:xo + int(a["xa_len"][i])].decode("latin-1") == xa and int(a["nm"][i]) == nm, i
    assert bool(res["flags"] & eng.SAMTEXT_PAIRED) == bool((a["flag5"] & 1).any()) == ("paired=1" in tail)
    assert bool(res["flags"] & eng.SAMTEXT_XA) == any_xa == ("xa=1" in tail)
    assert not res["flags"] & eng.SAMTEXT_NUL
    return res, a


# ---- 1. the ABI on built chunks ---------------------------------------------------------------------------------------------------

def test_empty_and_one_line(sam, dump, tmp_path):
    for final in (True, False):
        res = sam.parse(b"", final)
        assert (res["n_lines"], res["n_rec"], res["consumed"], res["n_hard"], res["flags"]) == (0, 0, 0, 0, 0)
    one = line(1, opt=("NM:i:2", XA1), flag="99")
    check_chunk(sam, dump, tmp_path, one[:-1], final=True, expect_lines=1)          # no newline, the input ends here: a line
    res = sam.parse(one[:-1], False)
    assert (res["n_lines"], res["n_rec"], res["consumed"], res["n_hard"]) == (0, 0, 0, 0)     # ... and more may come: nothing is consumed
    check_chunk(sam, dump, tmp_path, one, final=False, expect_lines=1)
    check_chunk(sam, dump, tmp_path, one + line(2, eol="\r\n"), final=True, expect_lines=2)


def line_of(i, total):
    """a plain line of exactly `total` bytes, newline included"""
    base = len(line(i, 30, opt=("ZZ:Z:",)))
    assert total >= base
    out = line(i, 30, opt=("ZZ:Z:" + "z" * (total - base),))
    assert len(out) == total
    return out


@pytest.mark.parametrize("at", [TILE - 1, TILE, TILE + 1, 2 * TILE - 1, 2 * TILE])
def test_newline_at_a_tile_boundary(at, sam, dump, tmp_path):
    text, i = b"", 0
    while len(text) + 500 < at:
        text += line(i, 30 + i % 50, opt=(XA1,) if i % 4 == 0 else ())
        i += 1
    text += line_of(i, at + 1 - len(text))                # its newline lands on byte `at`
    assert text[at:at + 1] == b"\n" and len(text) == at + 1
    for j in range(i + 1, i + 40):
        text += line(j, 20 + j % 30)
    check_chunk(sam, dump, tmp_path, text, expect_lines=i + 40)


@pytest.mark.parametrize("long_len", [40_000, 70_000])
def test_long_line_among_short_ones(long_len, sam, dump, tmp_path):
    """a line that spans three tiles, and a 70 000-base read: its wave's 64 lines do not fit the LDS window and are parsed out of global
    memory, the waves before and after out of LDS"""
    parts = [line(i, 30 + i % 40, opt=("NM:i:1", XA1) if i % 5 == 0 else ()) for i in range(150)]
    parts[100] = line(100, long_len, opt=("NM:i:3", XA1), flag="83")
    text = b"".join(parts)
    assert text.find(parts[100]) // TILE + 2 <= (text.find(parts[100]) + len(parts[100])) // TILE
    res, a = check_chunk(sam, dump, tmp_path, text, expect_lines=150)
    assert int(a["tmpend"][100]) == 1100 - 1 + long_len and int(a["xa_len"][100]) == len(XA1) - 5


@pytest.mark.parametrize("over", [0, 1, 16])
def test_sixty_four_lines_at_the_window_limit(over, sam, dump, tmp_path):
    """the first 64 lines take WIN + over bytes from the first line's first byte to the last line's last: at 0 they just fit"""
    parts = [line(i, 166) for i in range(63)]
    parts.append(line_of(63, WIN + over + 1 - sum(len(p) for p in parts)))
    assert sum(len(p) for p in parts) == WIN + over + 1 and len(parts[63]) < 1500
    text = b"".join(parts + [line(i, 40) for i in range(64, 200)])
    check_chunk(sam, dump, tmp_path, text, expect_lines=200)


def test_70001_records_and_two_slots(sam, dump, tmp_path):
    """more than 64 tiles, so the tile scan runs over more than one wave; and a second chunk parsed in the other slot meanwhile"""
    rng = np.random.default_rng(5)
    flags = ["0", "16", "99", "147", "4"]
    text = b"".join(line(i, 20 + i % 17, opt=(XA1, f"NM:i:{i % 7}") if i % 9 == 0 else (), flag=flags[int(rng.integers(5))]) for i in range(70_001))
    assert len(text) // TILE > 64 and len(text) <= MAX_CHUNK
    other = b"".join(line(i, 25) for i in range(333))
    sam.begin(text, True, 0)
    sam.begin(other + b"tail without newline", False, 1)
    r0, r1 = sam.end(0), sam.end(1)
    assert (r0["n_rec"], r0["n_hard"], r0["consumed"]) == (70_001, 0, len(text))
    assert (r1["n_rec"], r1["n_hard"], r1["consumed"]) == (333, 0, len(other))
    recs, _ = host_records(dump, text, tmp_path)
    host = np.array([[int(x) for x in r[:7]] for r in recs], np.int64)
    for first, n in ((0, 70_001), (69_999, 2), (4096, 4097)):
        a = sam.fetch(0, first, n)
        for k, name in enumerate(("tid", "pos", "tmpend", "mapq", "flag5", "mpos", "isize")):
            assert np.array_equal(a[name].astype(np.int64), host[first:first + n, k]), (name, first)
    a = sam.fetch(0, 0, 70_001)
    nl = np.flatnonzero(np.frombuffer(text, np.uint8) == 10)
    assert np.array_equal(a["line_off"][1:], nl[:-1] + 1) and a["line_off"][0] == 0
    b = sam.fetch(1, 0, 333, side=False)
    assert np.array_equal(b["pos"], 999 + np.arange(333))


def test_chunk_that_ends_in_mid_line(sam, dump, tmp_path):
    text = b"".join(line(i, 33, flag="65") for i in range(500))
    for cut in (len(text) - 1, len(text) - 40, len(text) // 2 + 7):
        res, _ = check_chunk(sam, dump, tmp_path, text[:cut], final=False)
        assert res["consumed"] < cut and res["n_lines"] == text[:cut].count(b"\n")


def _hard_kinds():
    kinds = [(k, l.encode("latin-1")) for k, (l, h) in named_cases().items() if h]
    assert len(kinds) >= 35
    return kinds


def test_one_hard_line_among_a_thousand(sam):
    plain = [line(i, 30 + i % 20) for i in range(1000)]
    kinds = _hard_kinds()
    for j, (kind, hard) in enumerate(kinds):
        at = (j * 131) % 1001
        text = b"".join(plain[:at]) + hard + b"".join(plain[at:])
        res = sam.parse(text, True)
        assert (res["n_hard"], res["first_hard_line"], res["n_rec"], res["n_lines"]) == (1, at, 0, 1001), (kind, res)
        assert bool(res["flags"] & eng.SAMTEXT_NUL) == (b"\0" in hard), kind
    # several: counted one by one, the first one named; a last line without newline
    text = b"".join(plain[:700]) + kinds[0][1] + b"".join(plain[700:900]) + kinds[3][1] + kinds[5][1] + b"".join(plain[900:]) + b"lonely"
    res = sam.parse(text, True)
    assert (res["n_hard"], res["first_hard_line"], res["n_rec"], res["n_lines"]) == (4, 700, 0, 1004)
    res = sam.parse(text, False)
    assert (res["n_hard"], res["first_hard_line"], res["n_lines"], res["consumed"]) == (3, 700, 1003, len(text) - 6)
    # lines too short to hold 11 fields, more of them than the record arrays have room for
    x = eng.SamText(NAMES, 4096)
    res = x.parse(b"a\n" * 2000, True)
    assert res["n_hard"] >= 1 and res["n_rec"] == 0 and res["consumed"] == 4000
    x.close()


def test_random_plain_lines_with_every_spelling(sam, dump, tmp_path):
    rng = np.random.default_rng(77)
    text = "".join(make_line(i, pick_plain(rng), "\r\n" if i % 13 == 0 else "\n")[0] for i in range(3000)).encode()
    check_chunk(sam, dump, tmp_path, text, expect_lines=3000)


def test_names_first_wins_and_no_names(dump, tmp_path):
    x = eng.SamText(NAMES, 1 << 16)
    res = x.parse(b"".join(line(i) for i in range(10)), True)
    assert res["n_rec"] == 10
    assert set(x.fetch(0, 0, 10)["tid"]) == {0, 1}                        # chr2 is reference 1, never 3
    x.close()
    none = eng.SamText([], 1 << 16)
    star = line(0).replace(b"\tchr2\t", b"\t*\t")
    res = none.parse(star * 3, True)
    assert res["n_rec"] == 3 and list(none.fetch(0, 0, 3)["tid"]) == [-1, -1, -1]
    res = none.parse(star + line(1), True)                                  # "missing header? Abort!" is the host's to say
    assert (res["n_hard"], res["first_hard_line"]) == (1, 1)
    none.close()


def test_argument_checks(sam):
    L = eng.load()
    h = C.c_void_p()
    off = np.array([0, 4], np.uint64)
    blob = np.frombuffer(b"chr1\0", np.uint8).copy()
    res = eng.SamTextResult()
    assert L.itx_samtext_create(0, eng._p(blob), eng._p(off), 1, 1 << 16, None) == -1
    assert L.itx_samtext_create(0, None, None, 1, 1 << 16, C.byref(h)) == -1
    assert L.itx_samtext_create(0, eng._p(blob), eng._p(off), -1, 1 << 16, C.byref(h)) == -1
    assert L.itx_samtext_create(0, eng._p(blob), eng._p(off), 1, 0, C.byref(h)) == -1
    assert L.itx_samtext_create(-1, eng._p(blob), eng._p(off), 1, 1 << 16, C.byref(h)) == -1
    assert L.itx_samtext_create(0, eng._p(blob), eng._p(off), 1, (256 << 20) + 1, C.byref(h)) == -6          # ITX_E_LIMIT
    assert L.itx_samtext_create(4096, eng._p(blob), eng._p(off), 1, 1 << 16, C.byref(h)) == -3               # ITX_E_NO_DEVICE
    assert not h.value
    L.itx_samtext_destroy(None)
    assert L.itx_samtext_parse_begin(None, 0, eng._p(blob), 4, 1) == -1
    assert L.itx_samtext_parse_begin(sam._h, 2, eng._p(blob), 4, 1) == -1
    assert L.itx_samtext_parse_begin(sam._h, 0, None, 4, 1) == -1
    assert L.itx_samtext_parse_begin(sam._h, 0, eng._p(blob), MAX_CHUNK + 1, 1) == -6
    assert L.itx_samtext_parse_end(None, 0, C.byref(res)) == -1 and L.itx_samtext_parse_end(sam._h, 0, None) == -1
    small = eng.SamText(NAMES, 1 << 16)
    assert L.itx_samtext_parse_end(small._h, 0, C.byref(res)) == -5                                           # nothing begun
    st = eng.Staging()
    assert L.itx_samtext_fetch(small._h, 0, 0, 0, C.byref(st), 0, *[None] * 6) == -1                           # a staging without arrays
    small.begin(line(1) * 5, True, 0)
    assert L.itx_samtext_parse_begin(small._h, 0, eng._p(blob), 4, 1) == -5                                   # begun twice
    with pytest.raises(eng.ItxError):
        small.fetch(0, 0, 1)                                                                                  # not ended yet
    assert small.end(0)["n_rec"] == 5
    with pytest.raises(eng.ItxError):
        small.fetch(0, 3, 3)                                                                                  # beyond the records
    with pytest.raises(eng.ItxError):
        small.fetch(1, 0, 1)                                                                                  # the other slot is empty
    assert L.itx_samtext_fetch(small._h, 0, 0, 5, None, 0, *[None] * 6) == -1
    assert len(small.fetch(0, 2, 3)["tid"]) == 3
    small.close()


# ---- 2. the command -----------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def exe():
    lib, exe = build.build_all()
    return exe


def _sam_line(err):
    m = re.search(r"\[itx timing\] sam: (\d+) chunks parsed on the device \((\d+) bytes, [0-9.]+ ms in its kernels, host waited [0-9.]+ s\), (\d+) by the host \((.*)\)", err)
    assert m, err[-1500:]
    return int(m.group(1)), int(m.group(3)), m.group(4)


def _user_stderr(err):
    return "\n".join(l for l in err.replace("\r", "\n").split("\n") if not l.startswith("[itx timing]") and "time used" not in l)


def _golden_sam_runs():
    runs = [(c, r) for c, r in gc.list_runs() if gc.manifest_run(c, r)["aln"].endswith(".sam")]
    return runs + [("addchr", "filter_C")]                              # the `filter -S -r` input of tests/test_gpu_names.py


@pytest.mark.parametrize("chunk", [4096, 1 << 20])
@pytest.mark.parametrize("case,run_name", _golden_sam_runs())
def test_sam_goldens_on_the_device_route(case, run_name, chunk, exe, tmp_path):
    run = gc.manifest_run(case, run_name)
    src = os.path.join(gc.GOLDEN, case, "in")
    opts = list(run["opts"])
    if not run["aln"].endswith(".sam"):
        opts = ["-S"] + opts
    paths = [refio.materialise(src, n, str(tmp_path)) for n in ["chrom.sizes", "rep.sizes", "rmsk.txt", "reads.sam"]]
    seen = {}
    for route in ("0", "1"):
        work = tmp_path / f"route{route}"
        work.mkdir()
        pr = subprocess.run([exe, run["cmd"]] + opts + ["-o", run["prefix"]] + paths, cwd=work, capture_output=True, text=True, timeout=600,
                            env=dict(os.environ, ITX_TIMING="1", ITX_SAM_CHUNK=str(chunk), ITX_HOST_SAM=route))
        assert pr.returncode == run["rc"], pr.stderr[-2000:]
        seen[route] = (work, pr.stderr)
    names = sorted(os.listdir(seen["0"][0]))
    assert names == sorted(os.listdir(seen["1"][0])) and names
    for fn in names:
        assert filecmp.cmp(seen["0"][0] / fn, seen["1"][0] / fn, shallow=False), fn
    if run["aln"].endswith(".sam"):
        for fn in run["files"]:
            assert (seen["0"][0] / fn).read_bytes() == refio.read_bytes(os.path.join(gc.GOLDEN, case, run_name, fn)), fn
    assert _user_stderr(seen["0"][1]) == _user_stderr(seen["1"][1])
    n_dev, n_host, why = _sam_line(seen["0"][1])
    h_dev, h_host, _ = _sam_line(seen["1"][1])
    print(case, run_name, chunk, "device chunks", n_dev, "host chunks", n_host, why)
    assert h_dev == 0 and h_host == n_dev + n_host >= 1
    if chunk == 4096:
        assert n_dev >= 1                               # (about one line in a hundred of these files has no CIGAR: a megabyte always holds one)


@pytest.fixture(scope="module")
def pile(tmp_path_factory):
    d = tmp_path_factory.mktemp("sam_pile")
    chroms = [("chr1", 2_000_000), ("chr2", 700_000)]
    t = synth.make_table(91, chroms, 3000, n_names=60, n_fams=9, n_clas=4, overlap_frac=0.05)
    synth.write_sizes(str(d / "chrom.sizes"), chroms)
    synth.write_sizes(str(d / "rep.sizes"), t.rep_len.items())
    synth.write_rmsk(str(d / "rmsk.txt"), t)
    r = synth.make_reads(92, chroms, 6000, read_len=(40, 120), paired_frac=0.3, nocigar_frac=0.0)
    rng = np.random.default_rng(93)
    r.aux = [[f"NM:i:{i % 3}", f"XA:Z:chr1,+{1 + int(rng.integers(1_900_000))},50M,1;"] if i % 4 == 0 else [] for i in range(len(r))]
    synth.write_sam(str(d / "reads.sam"), r)
    return d, t


def _stat(exe, d, out, opts, env, aln="reads.sam"):
    os.makedirs(out)
    pr = subprocess.run([exe, "stat", "-S"] + opts + ["-o", "out", str(d / "chrom.sizes"), str(d / "rep.sizes"), str(d / "rmsk.txt"), str(d / aln)], cwd=out,
                        capture_output=True, text=True, timeout=600, env=dict(os.environ, ITX_TIMING="1", **env))
    assert pr.returncode == 0, pr.stderr[-2000:]
    return pr.stderr


def _same_dirs(a, b):
    names = sorted(os.listdir(a))
    assert names and names == sorted(os.listdir(b))
    for fn in names:
        assert filecmp.cmp(os.path.join(a, fn), os.path.join(b, fn), shallow=False), fn


def test_plain_file_is_all_the_device(pile, exe, tmp_path):
    d, _ = pile
    size = os.path.getsize(d / "reads.sam")
    for k, opts in enumerate((["-w"], ["-w", "-x", "-B", "-V", "-R"])):
        dev = _stat(exe, d, str(tmp_path / f"dev{k}"), opts, {"ITX_HOST_SAM": "0", "ITX_SAM_CHUNK": "65536"})
        host = _stat(exe, d, str(tmp_path / f"host{k}"), opts, {"ITX_HOST_SAM": "1"})
        _same_dirs(str(tmp_path / f"dev{k}"), str(tmp_path / f"host{k}"))
        n_dev, n_host, why = _sam_line(dev)
        assert n_host == 0 and why == "none" and n_dev >= size // 65536
        assert _user_stderr(dev) == _user_stderr(host)
        assert "[itx timing] sam:" not in host          # getline: no chunks at all
    if os.path.exists(REF):
        os.makedirs(tmp_path / "ref")
        pr = subprocess.run([REF, "stat", "-S", "-w", "-x", "-B", "-V", "-R", "-o", "out", str(d / "chrom.sizes"), str(d / "rep.sizes"), str(d / "rmsk.txt"),
                             str(d / "reads.sam")], cwd=tmp_path / "ref", capture_output=True, text=True, timeout=600)
        assert pr.returncode == 0
        for fn in os.listdir(tmp_path / "ref"):
            if not fn.endswith(".bigWig"):
                assert filecmp.cmp(tmp_path / "ref" / fn, tmp_path / "dev1" / fn, shallow=False), fn


def test_unknown_reference_name_in_mid_file(pile, exe, tmp_path):
    """one line names a reference the header lacks: its chunk, and only that one, is the host's; the warning is the host route's"""
    d, _ = pile
    lines = open(d / "reads.sam").read().split("\n")
    k = len(lines) // 2
    f = lines[k].split("\t")
    f[2] = "chrNowhere"
    lines[k] = "\t".join(f)
    open(d / "odd.sam", "w").write("\n".join(lines))
    dev = _stat(exe, d, str(tmp_path / "dev"), ["-w"], {"ITX_HOST_SAM": "0", "ITX_SAM_CHUNK": "65536"}, aln="odd.sam")
    host = _stat(exe, d, str(tmp_path / "host"), ["-w"], {"ITX_HOST_SAM": "1"}, aln="odd.sam")
    _same_dirs(str(tmp_path / "dev"), str(tmp_path / "host"))
    n_dev, n_host, why = _sam_line(dev)
    assert n_host == 1 and n_dev >= 5 and f"line {k + 1} " in why, (n_dev, n_host, why)
    assert _user_stderr(dev) == _user_stderr(host)
    assert dev.count("[sam_read1] reference 'chrNowhere' is recognized as '*'.") == 1
