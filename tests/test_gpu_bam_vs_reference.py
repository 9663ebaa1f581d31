"""GPU: what the device wrote, checked by the reference's own BAM library (the samtools 0.1.18 it vendors) through
oracle/_ref/bamcheck (tests/refbam.py runs it; tests/test_bam_vs_reference.py pins the restatements against the same library
without a GPU).
1. the ABI: the shape cases of tests/test_gpu_bamidx.py (tests/baishapes.py), each wrapped as a file: a header member, the members
   engine.Bamout handed out, the EOF member. bam_index_build's index of the file equals the device's bytes under
   refbam.normalise, and bam_fetch through the device's bytes returns the linear scan's records for edge regions of the case;
2. the command, -b -i: the same two checks on the emitted pair, and the library's SAM text of our file equals its text of the input
   restricted to the counted records;
3. the command, -b -s -i: bam_sort_core leaves our order alone, its sort of the plain -b output agrees with ours up to the strand
   inside equal positions, and the index passes the checks of 2;
4. -l 0, -l 1 and -l 6 of one input give the library's BGZF reader the same text."""
import pytest

import baicase as bai
import baishapes as shapes
import refbam
from iteres_amd import synth
from test_bam_vs_reference import assert_same_up_to_the_strand, header
from test_gpu_bamidx import drive
from test_gpu_bamout import exe, oracle_rows, pile, raw_records, routes, run_filter   # noqa: F401  (fixtures and the synthetic inputs)
from test_gpu_bamsort import key_of, shuffled_bam

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not refbam.present, reason="oracle/_ref/bamcheck is not built (make -C oracle ref needs the reference tree)")]

BAM = "out_ALL.iteres.bam"

# ---- 1. the ABI

ABI_CASES = dict([("tile_%d_%s" % (n, hit), (lambda n=n, hit=hit: shapes.tile_boundaries(n, hit), None)) for n in (255, 256, 257) for hit in ("all", "third")] + [
    ("a_record_starts_on_the_last_byte_of_a_payload", (shapes.last_byte_of_a_payload, None)),
    ("chunks_merge", (lambda: shapes.bin_parent_bin_again(80), None)),
    ("chunks_do_not_merge", (lambda: shapes.bin_parent_bin_again(shapes.P + 900), None)),
    ("a_spliced_record_over_3000_windows", (shapes.spliced_over_3000_windows, None)),
    ("references_without_records", (shapes.references_without_records, None)),
    ("three_runs_with_host_appends", (shapes.big_case, 32768))])


@pytest.mark.parametrize("name", list(ABI_CASES))
def test_abi_index_and_fetch(name, tmp_path):
    make, cap = ABI_CASES[name]
    l_ref, steps = make()
    head = bai.bam_file(header(l_ref), [])[:-len(synth.BGZF_EOF)]            # the header's members: the record members begin behind them
    got, stream, status, idx, info = drive(l_ref, steps, first=len(head), cap=cap)
    assert status == bai.OK and info["entries"] == len(bai.records_of(stream)) > 0
    path = tmp_path / "case.bam"
    path.write_bytes(head + got + synth.BGZF_EOF)
    lib = refbam.check_index(path, idx)
    assert [r["meta"][1] for r in lib if r["meta"] is not None][-1] == (len(head) + len(got) + len(synth.BGZF_EOF)) << 16
    regions = refbam.edge_regions(path)
    hits = refbam.check_fetch(path, idx, regions)
    assert 6 <= hits < len(regions), (hits, len(regions))


# ---- 2. the command: -b -i

def check_pair(bam):
    """the library's index of the emitted file against the emitted .bai, and its fetch through the emitted .bai"""
    with open(str(bam) + ".bai", "rb") as f:
        ours = f.read()
    refbam.check_index(bam, ours)                                          # (bam_index_build writes over the .bai; check_fetch puts ours back)
    regions = refbam.edge_regions(bam)
    hits = refbam.check_fetch(bam, ours, regions)
    assert 10 <= hits < len(regions), (hits, len(regions))
    with open(str(bam) + ".bai", "rb") as f:
        assert f.read() == ours


@pytest.mark.parametrize("aln,opts", [("single.bam", ()), ("paired.bam", ("-R",)), ("mixed.bam", ())], ids=["single_ALL", "paired_R", "mixed_both_routes"])
def test_command_index_fetch_and_view(aln, opts, pile, exe, tmp_path):
    root, d, big, name = pile
    pr = run_filter(exe, d, str(tmp_path / "bi"), ("-b", "-i") + opts, d / aln, {"ITX_HOST_NAMES": "0"})
    assert "no index is written" not in pr.stderr
    bam = tmp_path / "bi" / BAM
    check_pair(bam)
    hit_row, locus_cnt = oracle_rows(root, aln, opts)
    head_in, lines_in = refbam.view(d / aln)
    head_out, lines_out = refbam.view(bam)
    assert head_out == head_in and lines_out == [ln for ln, h in zip(lines_in, hit_row) if h >= 0] and len(lines_out) == routes(pr.stderr)["records"] > 200


# ---- 3. the command: -b -s -i

def test_command_sort_against_the_librarys_sort(pile, exe, tmp_path):
    """mixed.bam shuffled (tests/test_gpu_bamsort.py), its chrU records as one run in the middle, so that both routes feed the sort"""
    root, d, big, name = pile
    head, recs = raw_records(d / "mixed.bam")
    shuffled_bam(tmp_path / "shuffled.bam", head, recs, 5, keep_together=lambda r: key_of(r)[0] == 1)
    env = {"ITX_HOST_NAMES": "0"}
    run_filter(exe, d, str(tmp_path / "bsi"), ("-b", "-s", "-i"), tmp_path / "shuffled.bam", env)
    run_filter(exe, d, str(tmp_path / "b"), ("-b",), tmp_path / "shuffled.bam", env)
    ours = raw_records(tmp_path / "bsi" / BAM)[1]
    assert len(ours) > 200 and max(key_of(r)[1] for r in ours) < 2 ** 31 - 1
    assert refbam.library_sort(tmp_path / "bsi" / BAM, tmp_path / "again")[1] == ours
    plain = raw_records(tmp_path / "b" / BAM)[1]
    by_lib = refbam.library_sort(tmp_path / "b" / BAM, tmp_path / "lib")[1]
    assert plain != ours and sorted(plain) == sorted(by_lib)
    assert_same_up_to_the_strand(ours, by_lib)
    check_pair(tmp_path / "bsi" / BAM)


# ---- 4. the levels

def test_levels_read_the_same_through_the_librarys_bgzf_reader(pile, exe, tmp_path):
    root, d, big, name = pile
    text = {}
    for level in ("0", "1", "6"):
        run_filter(exe, d, str(tmp_path / level), ("-b", "-l", level), d / "paired.bam", {"ITX_HOST_NAMES": "0"})
        text[level] = refbam.view(tmp_path / level / BAM)
    assert text["0"] == text["1"] == text["6"] and len(text["0"][1]) > 200
    assert len({(tmp_path / level / BAM).read_bytes() for level in text}) == 3   # three different files said the same
