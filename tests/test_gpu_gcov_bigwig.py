"""GPU: the bigWig content of `filter -W` at the C ABI (include/iteres_amd.h itx_gcov_bigwig_build / _result, csrc/itx_gcovbw.hip).
Intervals go in through itx_gcov_add_host (one case also through itx_gcov_run), the content comes back as packed zlib blocks and
summaries. Every section, every level's reduction and every zoom record are compared bit for bit with the model of
tests/bwsparse.py, and the digest of it all with the one recorded from the reference's converter (tests/golden/gcov_bigwig/,
held equal to a fresh run of the reference by tests/test_gcov_bigwig_cases.py). tests/gcovbwcases.py says what each case is for.

No input was found on which the reference drops a later level by its lastSummarySize comparison (it would need a level with twice
the summaries of the first reduction's last refused try; tests/test_gcov_bigwig_cases.py has the search), so no case pins that."""
import numpy as np
import pytest

import bwsparse as bs
import gcovbwcases as cases
import gcovcase as gv
from iteres_amd import engine as eng

pytestmark = pytest.mark.gpu

P0 = dict(extension=0, isize_max=500, treat_pe_as_se=False, discard_half_mapped=False, mapq_min=gv.MAPQ_MIN)


def open_case(key, host=True):
    chroms, iv = cases.case(key)
    idx = {n: i for i, (n, _) in enumerate(chroms)}
    g = eng.Gcov([s for _, s in chroms], P0, batch_capacity=1 << 16)
    if host:
        g.add_host([idx[c] for c, _, _, _ in iv], [s for _, s, _, _ in iv], [e for _, _, e, _ in iv], [u for _, _, _, u in iv])
    else:
        import torch
        g.set_tidmap(list(range(len(chroms))))
        dev = lambda a, t: torch.from_numpy(np.ascontiguousarray(a, t)).cuda()
        n = len(iv)
        g.run(dev(np.zeros(n), np.int32), dev([idx[c] for c, _, _, _ in iv], np.int32), dev([s for _, s, _, _ in iv], np.int32),
              dev([e for _, _, e, _ in iv], np.int32), dev([37 if u else 0 for _, _, _, u in iv], np.uint8), dev(np.zeros(n), np.uint8))
        g.wait_kernels()
    names = [n for n, _ in chroms]
    g.finish(sorted(range(len(names)), key=lambda i: names[i].encode()), names)
    return g, names, [s for _, s in chroms]


@pytest.fixture(scope="module")
def models():
    out = {}

    def get(key, w):
        if (key, w) not in out:
            sizes, per = cases.all_cases()[key]
            out[key, w] = bs.model(per[w], sizes) if any(per[w].values()) else None
        return out[key, w]
    return get


def check(res, names, sizes, m, recorded):
    d = bs.from_result(res, names, sizes)
    bs.check_against_model(d, m)
    assert bs.digest(d) == recorded
    assert res["n_items"] == sum(s[7] for s in m["sections"]) and res["reduce_rounds"] == m["rounds"]


@pytest.mark.parametrize("key", ["sections", "chain", "loop", "twoblocks"])
def test_content_is_the_reference_converters(key, models):
    g, names, sizes = open_case(key)
    rec = bs.recorded()
    for w in (0, 1):
        g.bigwig_build(w)
        res = g.bigwig(w)
        m = models(key, w)
        print(f"{key}/{w}: {res['n_items']} items, {len(res['sec_count'])} sections, reductions {res['reductions']}, "
              f"{[len(x) // 32 for x in res['sums']]} summaries, {res['reduce_rounds']} tries, ms {res['ms']}")
        check(res, names, sizes, m, rec[f"{key}/{w}"])
    st = g.stats()
    assert st["bw_items"] == [sum(s[7] for s in models(key, w)["sections"]) for w in (0, 1)]
    assert st["bw_sections"] == [len(models(key, w)["sections"]) for w in (0, 1)]
    assert st["bw_levels"] == [len(models(key, w)["zooms"]) for w in (0, 1)]
    assert st["bw_summaries"] == [sum(len(z[1]) // 32 for z in models(key, w)["zooms"]) for w in (0, 1)] and st["bw_ms"] > 0
    g.close()


def test_records_through_run_give_the_same_content(models):
    g, names, sizes = open_case("loop", host=False)
    g.bigwig_build(0)
    check(g.bigwig(0), names, sizes, models("loop", 0), bs.recorded()["loop/0"])
    g.close()


@pytest.mark.parametrize("order", ["before", "between", "after"])
def test_build_and_text_rounds_in_any_order(order, models):
    """the build reads the change points the text rounds read, and neither writes them"""
    chroms, iv = cases.case("sections")
    want = [gv.bedgraph([x[:3] for x in iv]), gv.bedgraph([x[:3] for x in iv if x[3]])]
    g, names, sizes = open_case("sections")
    text = [None, None]
    if order == "before":
        g.bigwig_build(0), g.bigwig_build(1)
        text = [g.text(0)[0], g.text(1)[0]]
    elif order == "between":
        text[0] = g.text(0)[0]
        g.bigwig_build(1), g.bigwig_build(0)
        text[1] = g.text(1)[0]
    else:
        text = [g.text(0)[0], g.text(1)[0]]
        g.bigwig_build(0), g.bigwig_build(1)
    assert text == want
    for w in (0, 1):
        check(g.bigwig(w), names, sizes, models("sections", w), bs.recorded()[f"sections/{w}"])
    g.close()


def test_a_file_without_data_has_no_content_and_the_other_is_unaffected(models):
    chroms, iv = cases.case("uniq_empty")
    g, names, sizes = open_case("uniq_empty")
    g.bigwig_build(1)
    assert g.bigwig(1) == {"n_items": 0}
    g.bigwig_build(0)
    check(g.bigwig(0), names, sizes, models("uniq_empty", 0), bs.recorded()["uniq_empty/0"])
    assert g.text(0)[0] == gv.bedgraph([x[:3] for x in iv]) and g.text(1)[0] == b""
    st = g.stats()
    assert st["bw_items"][1] == 0 and st["bw_sections"][1] == 0 and st["bw_levels"][1] == 0
    g.close()


def test_state_errors_follow_the_files_conventions():
    chroms, _ = cases.case("uniq_empty")
    g = eng.Gcov([s for _, s in chroms], P0, batch_capacity=1 << 16)
    g.add_host([1], [10], [20], [1])
    with pytest.raises(eng.ItxError, match="rc=-?[0-9]+: itx_gcov_bigwig_build: itx_gcov_finish comes first"):
        g.bigwig_build(0)
    g.finish([0, 1], [n for n, _ in chroms])
    with pytest.raises(eng.ItxError, match="itx_gcov_bigwig_build comes first"):
        g.bigwig(0)
    g.bigwig_build(0)
    with pytest.raises(eng.ItxError, match="has been built"):
        g.bigwig_build(0)
    res = g.bigwig(0)
    assert res["n_items"] == 1 and [tuple(k) for k in res["sec_key"]] == [(0, 10, 20)]
    assert (g.points(0) == np.array([[10, 1, 1, 0], [20, 0, 1, 0]], np.uint32)).all()
    assert g.text(0)[0] == b"chr2\t10\t20\t1\n"
    g.close()
