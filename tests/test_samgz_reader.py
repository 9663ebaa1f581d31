"""Host logic on CPU: -S input read through zlib (iteres_amd/host/samio.c sam_open), as the reference reads it (gzopen,
cussamtools/bam_import.c:17,76,126). The host reader (iteres_amd/host/test/reader_dump) must print the same records, byte for byte,
for a SAM text and for every compressed form of it: plain gzip, BGZF (a chain of gzip members), a mix of both, garbage behind the last
member; and, for a file cut short, what a streaming inflater gets out of the bytes that are left."""
import filecmp
import gzip
import os
import subprocess
import zlib

import numpy as np
import pytest

import goldencase as gc
import hosttool
import refio
from iteres_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.path.join(ROOT, "oracle", "_ref", "iteres")


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("bin") / "reader_dump")
    return hosttool.build(exe, "reader_dump.c")


def bgzf(text: bytes, payload: int, eof: bool = True, level: int = 6) -> bytes:
    out = b"".join(synth.bgzf_block(text[i:i + payload], level) for i in range(0, len(text), payload))
    return out + (synth.BGZF_EOF if eof else b"")


def inflate_what_is_there(data: bytes) -> bytes:
    """what a streaming inflater gets out of a chain of gzip members, the last of which may be cut short"""
    out, off = [], 0
    while off < len(data):
        d = zlib.decompressobj(31)
        try:
            out.append(d.decompress(data[off:]))
        except zlib.error:
            break
        if not d.eof:
            break
        off = len(data) - len(d.unused_data)
    return b"".join(out)


@pytest.fixture(scope="module")
def texts(tmp_path_factory):
    d = tmp_path_factory.mktemp("samgz_in")
    chroms = [("chr1", 2_000_000), ("chr2", 700_000)]
    r = synth.make_reads(411, chroms, 6000, read_len=(40, 120), paired_frac=0.3)
    rng = np.random.default_rng(412)
    r.aux = [[f"NM:i:{i % 3}", f"XA:Z:chr1,+{1 + int(rng.integers(1_900_000))},50M,1;"] if i % 4 == 0 else [] for i in range(len(r))]
    synth.write_sam(str(d / "synth.sam"), r)
    return {"quirks": refio.read_bytes(os.path.join(gc.GOLDEN, "quirks", "in", "reads.sam")), "synth": (d / "synth.sam").read_bytes()}


GARBAGE = b"\x00garbage\xff\x1f\x8b\x08\x00\x00"      # 14 bytes, a gzip magic among them


def forms(text: bytes):
    half = len(text) // 2
    return {
        "gzip1": gzip.compress(text, 1),
        "gzip9": gzip.compress(text, 9),
        "bgzf1000": bgzf(text, 1000),
        "bgzf1000_noeof": bgzf(text, 1000, eof=False),
        "bgzf_ff00": bgzf(text, 0xff00),
        "bgzf_ff00_noeof": bgzf(text, 0xff00, eof=False),
        "bgzf_then_gzip": bgzf(text[:half], 0xff00, eof=False) + gzip.compress(text[half:]),
        "gzip_then_garbage": gzip.compress(text) + GARBAGE,
    }


def run_dump(exe, path, chunk):
    env = {k: v for k, v in os.environ.items() if k not in ("ITX_SAM_CHUNK", "ITX_HOST_SAM")}
    if chunk:
        env["ITX_SAM_CHUNK"] = str(chunk)
    pr = subprocess.run([exe, str(path), "1", "4096"], capture_output=True, env=env)
    assert pr.returncode == 0, pr.stderr[-400:]
    return pr.stdout, pr.stderr


@pytest.mark.parametrize("chunk", [None, 4096])
@pytest.mark.parametrize("which", ["quirks", "synth"])
def test_same_dump_for_every_compression(which, chunk, texts, dump, tmp_path):
    text = texts[which]
    assert len(GARBAGE) == 14
    (tmp_path / "plain.sam").write_bytes(text)
    want = run_dump(dump, tmp_path / "plain.sam", chunk)
    assert want[0].count(b"\n") > 30 and b"#records=0 " not in want[0]
    for name, data in forms(text).items():
        p = tmp_path / f"{name}.sam.gz"
        p.write_bytes(data)
        got = run_dump(dump, p, chunk)
        assert got[0] == want[0], name
        assert got[1] == want[1], name


@pytest.mark.parametrize("chunk", [None, 4096])
def test_truncated_bgzf_gives_what_the_inflater_gets(chunk, texts, dump, tmp_path):
    text = texts["synth"]
    whole = bgzf(text, 0xff00)
    cut = whole[: len(whole) * 3 // 5]
    part = inflate_what_is_there(cut)
    assert 0 < len(part) < len(text) and text.startswith(part) and not part.endswith(b"\n")      # inside a member, inside a line
    (tmp_path / "cut.sam.gz").write_bytes(cut)
    (tmp_path / "part.sam").write_bytes(part)
    assert run_dump(dump, tmp_path / "cut.sam.gz", chunk) == run_dump(dump, tmp_path / "part.sam", chunk)


def test_reference_binary_reads_them_the_same(texts, dump, tmp_path):
    """the golden as BGZF and as BGZF followed by plain gzip: this reader's dump is the plain text's, and, where the reference binary is
    built, `stat -S -w` of the reference writes the files it writes for the plain text"""
    src = os.path.join(gc.GOLDEN, "quirks", "in")
    side = [refio.materialise(src, n, str(tmp_path)) for n in ("chrom.sizes", "rep.sizes", "rmsk.txt")]
    text = texts["quirks"]
    f = forms(text)
    inputs = {"plain": text, "bgzf": f["bgzf_ff00"], "mixed": f["bgzf_then_gzip"]}
    for name, data in inputs.items():
        (tmp_path / name).mkdir()
        (tmp_path / f"{name}.sam").write_bytes(data)
    want = run_dump(dump, tmp_path / "plain.sam", None)
    assert b"#records=0 " not in want[0]
    assert run_dump(dump, tmp_path / "bgzf.sam", None) == want and run_dump(dump, tmp_path / "mixed.sam", None) == want
    if not os.path.exists(REF):
        return
    for name in inputs:
        pr = subprocess.run([REF, "stat", "-S", "-w", "-o", "out"] + side + [str(tmp_path / f"{name}.sam")], cwd=tmp_path / name, capture_output=True, timeout=600)
        assert pr.returncode == 0, pr.stderr[-400:]
    names = sorted(os.listdir(tmp_path / "plain"))
    assert names
    for name in ("bgzf", "mixed"):
        assert sorted(os.listdir(tmp_path / name)) == names
        for fn in names:
            assert filecmp.cmp(tmp_path / "plain" / fn, tmp_path / name / fn, shallow=False), (name, fn)
