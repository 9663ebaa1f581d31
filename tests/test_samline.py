"""The SAM line rule stated once (iteres_amd/csrc/itx_samline.h, built for the host by tests/samline_host.cpp) against the
product's own SAM parser (iteres_amd/host/samio.c through iteres_amd/host/test/reader_dump) on the same file: every line the
rule does not call hard gives the same tid pos tmpend mapq flag5 mpos isize qname, every line written in a spelling only the
host models is called hard, and the rule cannot pass by calling everything hard. Then the reader's two line iterators — getline,
and lines taken out of chunks in memory — against each other."""
import os
import re
import subprocess

import numpy as np
import pytest

import goldencase as gc
import hosttool
import refio

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = "@HD\tVN:1.0\n@SQ\tSN:chr1\tLN:1000000\n@SQ\tSN:chr2\tLN:500000\n@SQ\tSN:chrX\tLN:200000\n@SQ\tSN:chr2\tLN:7\n@PG\tID:x\n"


@pytest.fixture(scope="module")
def tools(tmp_path_factory):
    d = tmp_path_factory.mktemp("bin")
    dump, rule = str(d / "reader_dump"), str(d / "samline_host")
    hosttool.build(dump, "reader_dump.c")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-o", rule, os.path.join(ROOT, "tests", "samline_host.cpp")])
    return dump, rule


# ---- spellings: (text, hard) per field ----------------------------------------------------------------------------------------
FLAG = [("0", 0), ("4", 0), ("16", 0), ("99", 0), ("147", 0), ("83", 0), ("1024", 0), ("65", 0), ("999999999", 0),
        ("00", 1), ("04", 1), ("0x10", 1), ("+4", 1), ("-1", 1), (" 4", 1), ("4 ", 1), ("pP", 1), ("", 1), ("1234567890", 1)]
RNAME = [("*", 0), ("chr1", 0), ("chr2", 0), ("chrX", 0), ("chrUn", 1), ("", 1), ("chr1 ", 1)]
POS = [("0", 0), ("1", 0), ("12345", 0), ("12x", 0), ("x12", 0), ("-5", 0), ("", 0), ("999999999", 0), ("007", 0), ("1234567890", 1)]
MAPQ = [("0", 0), ("60", 0), ("255", 0), ("300", 0), ("x", 0), ("", 0), ("37", 0), ("12345678901", 1)]
CIGAR = [("50M", 0), ("10m5d3n", 0), ("5S40M5S", 0), ("3H10M", 0), ("10M2I10M", 0), ("10=2X", 0), ("5P7M", 0), ("", 0), ("123456789M", 0), ("4M1000000N4M", 0),
         ("M", 1), ("10", 1), ("10M5", 1), ("+5M", 1), ("-5M", 1), (" 5M", 1), ("5 M", 1), ("1234567890M", 1)]
PNEXT = [("0", 0), ("1", 0), ("777", 0), ("9y", 0), ("", 0), ("*", 0), ("1234567890", 1)]
TLEN = [("0", 0), ("100", 0), ("-100", 0), ("-", 0), ("-x", 0), ("x", 0), ("+5", 0), ("", 0), ("--5", 0), ("12z", 0), ("1234567890", 1), ("-1234567890", 1)]
SEQ = [("*", 0), ("ACGT" * 9, 0), ("A", 0), ("*A", 0), ("", 0), ("ACGTN" * 20, 0)]
XA1 = "XA:Z:chr1,+100,50M,1;chr2,-7,50M,0;"
OPT = [([], 0), (["NM:i:2"], 0), ([XA1], 0), (["NM:i:1", XA1], 0), ([XA1, "NM:i:3"], 0), (["AS:i:30", XA1, "MD:Z:50"], 0), (["XA:i:3"], 0), (["XA:Z"], 0),
       (["XA:Z:"], 0), (["XA:H:1AE3"], 0), ([XA1, "XA:Z:second"], 0), ([XA1, "NM:i:-3"], 0), ([XA1, "NM:Z:x"], 0), ([XA1, "NM:i"], 0), (["NM:i:+3"], 0),
       (["NM:i:7", "NM:i:8", XA1], 0), (["XA", "XA:", "X"], 0), (["AS:i:1", "XA:Z"], 0), (["NM:i:12x", XA1], 0), ([""], 0),
       ([XA1, "NM:i:+3"], 1), (["NM:i:", XA1], 1), ([XA1, "NM:i:x"], 1), ([XA1, "NM:i:1234567890"], 1), (["NM:i: 3", XA1], 1)]
FIELDS = [FLAG, RNAME, POS, MAPQ, CIGAR, PNEXT, TLEN, SEQ, OPT]


def make_line(i, picks, eol="\n"):
    """picks: one (text, hard) per entry of FIELDS; returns (line with its terminator, hard)"""
    flag, rname, pos, mapq, cigar, pnext, tlen, seq, opt = [p[0] for p in picks]
    f = [f"r{i}", flag, rname, pos, mapq, cigar, "=", pnext, tlen, seq, "*" if seq in ("*", "") else "I" * len(seq)] + list(opt)
    return "\t".join(f) + eol, int(any(p[1] for p in picks))


def plain(field):
    return [s for s in field if not s[1]]


def pick_plain(rng):
    return [f[int(rng.integers(len(plain(f))))] for f in map(plain, FIELDS)]


def star_cigar(picks, flag):
    """the same line with CIGAR `*` and the given flag"""
    q = list(picks)
    q[0] = (flag, 0)
    q[4] = ("*", 0)
    return q


def named_cases():
    base = [("99", 0), ("chr1", 0), ("1000", 0), ("60", 0), ("50M", 0), ("1200", 0), ("250", 0), ("ACGT" * 9, 0), ([], 0)]
    cases = {}
    for k, field in enumerate(FIELDS):
        for j, sp in enumerate(field):
            q = list(base)
            q[k] = sp
            cases[f"field{k}_{j}"] = make_line(len(cases), q)
    cases["star_cigar_unmapped"] = make_line(len(cases), star_cigar(base, "4"))
    cases["star_cigar_unmapped_tail"] = (make_line(len(cases), star_cigar(base, "77"))[0].replace("\t*\t=", "\t*zz\t="), 0)
    cases["star_cigar_mapped"] = (make_line(len(cases), star_cigar(base, "0"))[0], 1)
    cases["star_cigar_mapped_99"] = (make_line(len(cases), star_cigar(base, "99"))[0], 1)
    cases["exactly_11_fields"] = make_line(len(cases), base)
    cases["crlf"] = make_line(len(cases), base, "\r\n")
    cases["crcrlf_xa_last"] = make_line(len(cases), base[:8] + [(["NM:i:4", XA1], 0)], "\r\r\n")
    cases["xa_z_at_the_very_end_crlf"] = make_line(len(cases), base[:8] + [(["XA:Z"], 0)], "\r\n")
    cases["ten_fields"] = ("\t".join(["short", "0", "chr1", "5", "9", "5M", "=", "0", "0", "ACGTA"]) + "\n", 1)
    cases["one_field"] = ("lonely\n", 1)
    cases["empty_line"] = ("\n", 1)
    cases["only_cr"] = ("\r\n", 1)
    cases["nul_in_seq"] = (make_line(len(cases), base)[0].replace("ACGTACGT", "ACGT\0CGT", 1), 1)
    cases["nul_in_aux"] = (make_line(len(cases), base[:8] + [([XA1], 0)])[0].replace("50M,1;", "50M\0,1;", 1), 1)
    cases["mapq_300"] = make_line(len(cases), base[:3] + [("300", 0)] + base[4:])
    cases["qname_odd"] = ("a b:c/1#x\t" + make_line(0, base)[0].split("\t", 1)[1], 0)
    return cases


def random_lines(n, seed):
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        picks = pick_plain(rng)
        u = rng.random()
        if u < 0.08:                                   # one field of the line in a spelling only the host models
            k = int(rng.integers(len(FIELDS)))
            hard = [s for s in FIELDS[k] if s[1]]
            if hard:
                picks[k] = hard[int(rng.integers(len(hard)))]
        elif u < 0.16:                                 # no CIGAR: plain on an unmapped record (hard on a mapped one: below)
            picks = star_cigar(picks, ("4", "77", "141", "12")[int(rng.integers(4))])
        elif u < 0.17:
            line, _ = make_line(i, star_cigar(picks, ("0", "16", "99")[int(rng.integers(3))]))
            out.append((line, 1))
            continue
        eol = "\r\n" if rng.random() < 0.05 else "\n"
        out.append(make_line(i, picks, eol))
    return out


def expect_aux(line):
    """(has_xa, nm, xa) as samio.c reads a plain line's optional fields"""
    body = line.rstrip("\r\n")
    f = body.split("\t", 11)
    if len(f) < 12:
        return 0, 0, ""
    rest, xa, nm = f[11], None, None
    for st in [0] + [m.end() for m in re.finditer("\t", rest)]:
        if xa is None and rest.startswith("XA:", st):
            xa = rest[st:]
        if nm is None and rest.startswith("NM:", st):
            nm = rest[st:]
    if xa is None:
        return 0, 0, ""
    v = xa[5:].split("\t")[0] if len(xa) >= 5 and xa[3] in "ZH" and xa[4] == ":" else ""
    n = 0
    if nm is not None and len(nm) >= 5 and nm[3] == "i" and nm[4] == ":":
        n = int(re.match(r"-?[0-9]+", nm[5:]).group())
    return 1, n, v


def run_rule(rule, path):
    pr = subprocess.run([rule, path], capture_output=True)
    assert pr.returncode == 0, pr.stderr
    return [l for l in pr.stdout.decode("latin-1").split("\n")[:-1] if not l.startswith("@")]


def run_dump(dump, path, batch=4096, env=None):
    e = dict(os.environ, OMP_NUM_THREADS="2")
    for k in ("ITX_SAM_CHUNK", "ITX_HOST_SAM"):
        e.pop(k, None)
    e.update(env or {})
    pr = subprocess.run([dump, path, "1", str(batch)], capture_output=True, env=e)
    assert pr.returncode == 0, pr.stderr
    return pr.stdout.decode("latin-1"), pr.stderr.decode("latin-1")


@pytest.fixture(scope="module")
def corpus(tools, tmp_path_factory):
    """the named cases, then 20 000 random lines: (lines, rule's output per line, number of named cases, directory)"""
    dump, rule = tools
    d = tmp_path_factory.mktemp("sam")
    named = named_cases()
    lines = list(named.values()) + random_lines(20000, 20240607)
    path = str(d / "all.sam")
    with open(path, "w", newline="") as f:
        f.write(HEADER + "".join(l for l, _ in lines))
    got = run_rule(rule, path)
    assert len(got) == len(lines)
    return lines, got, list(named), str(d)


def test_named_cases(corpus):
    lines, got, names, _ = corpus
    for name, (line, hard), g in zip(names, lines, got):
        assert (g == "H") == bool(hard), (name, line, g)


def test_hard_lines_are_called_hard_and_few(corpus):
    lines, got, names, _ = corpus
    rnd, rgot = lines[len(names):], got[len(names):]
    assert len(rnd) == 20000
    for (line, hard), g in zip(rnd, rgot):
        assert (g == "H") == bool(hard), (line, g)
    # the cap holds for the spellings as written (what the host parser alone would need) and for what the rule calls hard
    assert sum(h for _, h in rnd) <= 2000
    assert sum(g == "H" for g in rgot) <= 2000
    assert sum(g == "H" for g in rgot) >= 200            # and the hard spellings are really drawn


def test_plain_lines_equal_the_host_parser(corpus, tools):
    dump, _ = tools
    lines, got, names, d = corpus
    keep = [(l, g) for (l, _), g in zip(lines, got) if g != "H"]
    path = os.path.join(d, "plain.sam")
    with open(path, "w", newline="") as f:
        f.write(HEADER + "".join(l for l, _ in keep))
    out, err = run_dump(dump, path)
    assert "recognized as" not in err and "Parse warning" not in err and "Abort" not in err, err[:400]
    recs = [l for l in out.split("\n") if l and l[0] not in "@#"]
    assert len(recs) == len(keep)
    for (line, g), rec in zip(keep, recs):
        cols = g.split("\t")
        assert cols[:8] == rec.split("\t"), (line, g, rec)
        has_xa, nm, xa = expect_aux(line)
        assert int(cols[8]) == has_xa, (line, g)
        if has_xa:
            assert int(cols[9]) == nm and cols[10] == xa, (line, g)
    tail = [l for l in out.split("\n") if l.startswith("#")][0]
    assert f"paired={int(any(int(g.split(chr(9))[4]) & 1 for _, g in keep))}" in tail
    assert f"xa={int(any(g.split(chr(9))[8] == '1' for _, g in keep))}" in tail


def _sam_goldens():
    return sorted(c for c in os.listdir(gc.GOLDEN)
                  if os.path.exists(os.path.join(gc.GOLDEN, c, "in", "reads.sam")) or os.path.exists(os.path.join(gc.GOLDEN, c, "in", "reads.sam.gz")))


@pytest.mark.parametrize("case", _sam_goldens())
def test_chunk_iterator_equals_getline_on_goldens(case, tools, tmp_path):
    dump, _ = tools
    path = refio.materialise(os.path.join(gc.GOLDEN, case, "in"), "reads.sam", str(tmp_path))
    want = run_dump(dump, path)
    assert "#records=" in want[0]
    for chunk, batch in ((4096, 4096), (4096, 777), (50, 4096), (1 << 20, 333)):      # 50: every line is longer than a chunk
        assert run_dump(dump, path, batch, {"ITX_SAM_CHUNK": str(chunk), "ITX_HOST_SAM": "1"}) == want, (chunk, batch)


def test_chunk_iterator_equals_getline_on_odd_lines(corpus, tools):
    """warnings with their line numbers, skipped lines and the batch a truncated line ends: the same from memory as from getline"""
    dump, _ = tools
    _, _, _, d = corpus
    path = os.path.join(d, "all.sam")
    want = run_dump(dump, path, 500)
    assert "Parse warning at line" in want[1] and "recognized as" in want[1]
    for chunk in (4096, 100_000):
        assert run_dump(dump, path, 500, {"ITX_SAM_CHUNK": str(chunk), "ITX_HOST_SAM": "1"}) == want, chunk
