"""The tag walk stated once (iteres_amd/csrc/itx_auxwalk.h) built for the host (tests/auxwalk_host.cpp, a program of its own)
against the literal model of the reference's walk (tests/auxmodel.py, itself held to the reference binary by
tests/test_auxwalk_vs_reference.py): on the three sets of tests/auxcases.py — where the reference is undefined, the project's own
rule answers: the walk stops, the tag counts as not found, a value or string that would run past the end reads as 0 or empty —
and on seeded byte-fuzzed optional fields. Every record lies in a heap block of exactly its size, and the same program built with
-fsanitize=address,undefined must report nothing. The header is plain C as well: gcc -std=gnu11 takes it."""
import os
import struct
import subprocess

import numpy as np
import pytest

import auxcases as ac
import auxmodel as am
from bedcase import record

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "auxwalk_host.cpp")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def prog(request, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("auxwalk") / ("auxwalk_host_" + request.param))
    subprocess.check_call(["g++", "-O1" if request.param == "sanitized" else "-O2", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror"] +
                          (SAN if request.param == "sanitized" else []) + ["-o", exe, SRC])
    return exe


def fuzzed(seed, n):
    """optional fields of the cases with bytes changed, cut, doubled or made up, each behind a record header of its own"""
    rng = np.random.default_rng(seed)
    base = [r for r in ac.cases()[0] if r.aux]
    interesting = np.frombuffer(b"XANMZHBfdcCsSiIA\0\0\0\1\xff;,", np.uint8)
    out = []
    for i in range(n):
        a = bytearray(base[int(rng.integers(0, len(base)))].aux)
        how = rng.random()
        if how < 0.5:
            for _ in range(int(rng.integers(1, 4))):
                a[int(rng.integers(0, len(a)))] = int(rng.choice(interesting)) if rng.random() < 0.7 else int(rng.integers(0, 256))
        elif how < 0.7:
            a = a[:int(rng.integers(0, len(a) + 1))]
        elif how < 0.8:
            k = int(rng.integers(0, len(a)))
            a = a[:k] + a[k:k + int(rng.integers(1, 6))] + a[k:]
        elif how < 0.9:
            a = bytearray(int(x) for x in rng.choice(interesting, int(rng.integers(0, 40))))
        else:
            a = bytearray(int(x) for x in rng.integers(0, 256, int(rng.integers(0, 24))))
        kw = [dict(), dict(l_qseq=7), dict(cigar=(), l_qseq=0), dict(cigar=((0, 20), (1, 5), (0, 30)), l_qseq=55)][i % 4]
        out.append(record(qname=b"f%d\0" % i, aux=bytes(a), **kw))
    return out


def run(prog, recs, tmp_path):
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    src.write_bytes(b"".join(struct.pack("<I", len(r)) + r for r in recs))
    pr = subprocess.run([prog, str(src), str(dst)], capture_output=True, text=True, timeout=120,
                        env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1"))
    assert pr.returncode == 0 and pr.stderr == "", pr.stderr[-3000:]
    b, at, got = dst.read_bytes(), 0, []
    for _ in recs:
        has, nm, xl = struct.unpack_from("<BiI", b, at)
        got.append((bool(has), nm, b[at + 9:at + 9 + xl]))
        at += 9 + xl
    assert at == len(b)
    return got


def test_header_gives_the_models_answer_on_the_three_sets(prog, tmp_path):
    R, _ = ac.cases()
    got = run(prog, [r.rec for r in R], tmp_path)
    wrong = [(r.label, r.set, r.aux, g, (r.a.has_xa, r.a.p_nm, r.a.p_xa)) for r, g in zip(R, got) if g != (r.a.has_xa, r.a.p_nm, r.a.p_xa)]
    assert not wrong, (len(wrong), wrong[:5])
    # the sets are all there, and the undefined one holds every way of leaving the record
    sets = {s: sum(r.set == s for r in R) for s in ("ref_safe", "all_defined", "undefined")}
    assert sets["ref_safe"] > 3000 and sets["all_defined"] >= 10 and sets["undefined"] >= 100, sets
    und = [r for r in R if r.set == "undefined"]
    assert any(r.a.found is am.UNDEF for r in und) and any(r.a.nm is am.UNDEF for r in und) and any(r.a.xa is am.UNDEF for r in und)


def test_header_gives_the_models_answer_on_fuzzed_fields(prog, tmp_path):
    recs = fuzzed(77, 20_000)
    got = run(prog, recs, tmp_path)
    ans = [am.answer(r) for r in recs]
    wrong = [(am.aux_region(r), g, (a.has_xa, a.p_nm, a.p_xa)) for r, g, a in zip(recs, got, ans) if g != (a.has_xa, a.p_nm, a.p_xa)]
    assert not wrong, (len(wrong), wrong[:5])
    n_und = sum(a.undefined for a in ans)
    assert n_und > 1000 and sum(a.has_xa for a in ans) > 5000 and sum(a.found is True and a.xa is None for a in ans) > 20, n_und


def test_header_is_plain_c(tmp_path):
    src = tmp_path / "one.c"
    src.write_text('#include "%s"\nint main(void) { return 0; }\n' % os.path.join(ROOT, "iteres_amd", "csrc", "itx_auxwalk.h"))
    subprocess.check_call(["gcc", "-std=gnu11", "-Wall", "-Wextra", "-Werror", "-Wno-unused-function", "-o", str(tmp_path / "one"), str(src)])


def test_one_walk_in_the_package():
    """the type sizes of the walk are written down in one file of iteres_amd/"""
    import re
    hits = []
    for d, _, files in os.walk(os.path.join(ROOT, "iteres_amd")):
        for fn in files:
            if fn.endswith((".h", ".hip", ".c", ".cpp")):
                text = open(os.path.join(d, fn), errors="replace").read()
                if re.search(r"type == 'Z' \|\| type == 'H'", text):
                    hits.append(fn)
    assert hits == ["itx_auxwalk.h"], hits
