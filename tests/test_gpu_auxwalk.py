"""GPU: the reference's tag walk on the device, record by record against its literal model (tests/auxmodel.py, held to the reference
binary by tests/test_auxwalk_vs_reference.py) — through the C ABI in windows of 1, 63, 64, 65, 255, 256 and 257 records and one of
all of them (tests/auxcases.py: every tag type in front of, between and behind NM and XA, floats whose bytes spell tags, records
that end inside a tag):

    itx_bamwin_push / parse / fetch   the XA marks are the model's "found"
    itx_bamwin_bed (itx_bed_run)      every -B line is the model's line
    itx_xaveto_* / itx_bamwin_xa_veto the chosen rows in the veto object's buffer as the command puts them there; NOLOOKUP per record,
                                      n_vetoed and n_hard are the model's; a window with a record for the host marks nothing

and through the command on the records the reference is defined on: the device's reading of the tags equals the host's
(ITX_HOST_VETO=1) and, where it is built, the reference binary's files."""
import filecmp
import os

import numpy as np
import pytest

import auxcases as ac
import auxmodel as am
import bedcase as bc
from iteres_amd import build, engine as eng
from test_gpu_bed import fetch, window
from test_gpu_xaveto import _routes, _run, _vetoed

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.path.join(ROOT, "oracle", "_ref", "iteres")
P = bc.params()


class Rig:
    """the table of tests/auxcases.py on the device, an engine, the veto object and the bed object over it"""

    def __init__(self):
        self.R, self.n = ac.cases()
        rows, self.model_table = ac.table(self.n)
        self.header = ac.chroms(self.n)
        names = list(dict.fromkeys(nm for _, _, _, nm in rows))
        rep = {nm: i for i, nm in enumerate(names)}
        word = {}
        rep_word = [word.setdefault(nm.upper(), len(word)) for nm in names]
        m = len(rows)
        r = eng.make_rows([c for c, _, _, _ in rows], [s for _, s, _, _ in rows], [e for _, _, e, _ in rows], np.zeros(m), [e - s for _, s, e, _ in rows],
                          [rep[nm] for _, _, _, nm in rows], np.zeros(m, np.int64), np.zeros(m, np.int64))
        sizes = np.array([l for _, l in self.header], np.int64)
        self.tab = eng.Table(r, sizes, np.full(len(names), 600, np.uint32), 1, 1)
        self.eng = eng.Engine(self.tab, P, batch_capacity=1 << 13)
        self.eng.set_tidmap([0, 1, 2])
        self.xv = eng.XaVeto(self.eng, [rep[nm] for _, _, _, nm in rows], rep_word, [nm for nm, _ in self.header], batch_capacity=1 << 13)
        self.xv.set_tidmap([0, 1, 2])
        self.bed = eng.Bed(sizes, P, want=eng.BED_ALL, batch_capacity=1 << 13)
        self.bed.set_tidmap([0, 1, 2], [nm for nm, _ in self.header])
        self.inf = eng.Inflater()
        self.judged = dict(zip((r.k for r in self.R), device_verdicts(self, self.R)))       # the model's verdicts, once

    def close(self):
        for o in (self.inf, self.bed, self.xv, self.eng, self.tab):
            o.close()


@pytest.fixture(scope="module")
def rig():
    r = Rig()
    yield r
    r.close()


def spread(recs, w):
    return recs if w >= len(recs) else [recs[i * len(recs) // w] for i in range(w)]


def device_verdicts(rig, recs):
    return [ac.verdict(r, rig.model_table, rig.n, P["extension"], device=True) for r in recs]


@pytest.mark.parametrize("w", [1, 63, 64, 65, 255, 256, 257, 1 << 20], ids=lambda w: "all" if w == 1 << 20 else str(w))
def test_marks_lines_and_verdicts_are_the_models(rig, w):
    """all_defined and undefined records, without the few that are the host's to judge (they have a test of their own below)"""
    recs = spread([r for r in rig.R if rig.judged[r.k][1] is not am.HARD], w)
    assert len(recs) == w or (w == 1 << 20 and len(recs) > 6000)
    if w >= 63:
        assert {r.set for r in recs} >= ({"ref_safe", "all_defined", "undefined"} if w == 1 << 20 else {"ref_safe", "undefined"})
    n = window(rig.inf, bc.bam_bytes(rig.header, [r.rec for r in recs]))
    assert n == len(recs)
    # ---- the XA marks of the parse
    arrs, _ = fetch(rig.inf, n)
    xa = np.zeros(n, np.uint8)
    off = np.zeros(n, np.uint32)
    st = eng.Staging(*[arrs[k].ctypes.data for k in ("tid", "pos", "tmpend", "mapq", "flag5", "mpos", "isize")], None, n)
    eng._chk(eng.load().itx_bamwin_fetch(rig.inf._h, 0, n, st, 0, eng._p(off), eng._p(xa)), "fetch")
    want_xa = np.array([r.a.has_xa for r in recs])
    wrong = [(recs[i].label, recs[i].aux) for i in np.flatnonzero((xa != 0) != want_xa)]
    assert not wrong, (len(wrong), wrong[:5])
    # ---- the -B lines
    assert rig.bed.start_window(rig.inf, 0, n) == 0
    got = rig.bed.collect()[0].split(b"\n")
    want = bc.lines(P, rig.header, [nm for nm, _ in rig.header], [l for _, l in rig.header], [r.rec for r in recs])[0].split(b"\n")
    assert len(got) == len(want) == n + 1
    wrong = [(r.label, r.aux, g, x) for r, g, x in zip(recs, got, want) if g != x]
    assert not wrong, (len(wrong), wrong[:5])
    # ---- the veto
    want_v = [rig.judged[r.k] for r in recs]
    n_vetoed, n_hard = rig.xv.judge(rig.inf, 0, n)
    f5 = fetch(rig.inf, n)[0]["flag5"]
    marked = (f5 & eng.F5_NOLOOKUP) != 0
    want_m = np.array([bool(c and v is True) for c, v in want_v])
    wrong = [(recs[i].label, recs[i].aux, bool(marked[i])) for i in np.flatnonzero(marked != want_m)]
    assert not wrong, (len(wrong), wrong[:5])
    assert (n_vetoed, n_hard) == (int(want_m.sum()), 0)
    if w >= 255:
        assert 0 < want_m.sum() < n and sum(r.a.old_walk_differs(r.aux) for r in recs) >= 0.02 * n


def test_a_window_with_records_for_the_host_marks_nothing(rig):
    """every record, the ones with numbers only strtol reads and alternatives without four fields among them: n_hard is the
    model's count and no record is marked; then the same window with ONE such record"""
    hard = [r for r in rig.R if rig.judged[r.k][0] and rig.judged[r.k][1] is am.HARD]
    assert len(hard) >= 8
    plain = [r for r in rig.R if rig.judged[r.k][1] is not am.HARD][:700]
    for recs, n_want in ((rig.R, len(hard)), (plain[:300] + hard[:1] + plain[300:], 1)):
        n = window(rig.inf, bc.bam_bytes(rig.header, [r.rec for r in recs]))
        assert n == len(recs)
        n_vetoed, n_hard = rig.xv.judge(rig.inf, 0, n)
        assert (n_vetoed, n_hard) == (0, n_want)
        assert not (fetch(rig.inf, n)[0]["flag5"] & eng.F5_NOLOOKUP).any()
        assert sum(bool(c and v is True) for c, v in (rig.judged[r.k] for r in recs)) > 50          # there was something to mark


# ---- the command

@pytest.fixture(scope="module")
def safe_case(tmp_path_factory):
    d = tmp_path_factory.mktemp("auxwalk_cmd")
    ac.write_inputs(d, ac.subset(("ref_safe",)), ac.cases()[1])
    return d


@pytest.mark.parametrize("opts", [("-w", "-B"), ("-w", "-T", "-E", "0")], ids=["wB", "wTE0"])
def test_command_device_equals_host_and_reference(opts, safe_case, tmp_path):
    exe = build.build_all()[1]
    dev = _run(exe, safe_case, str(tmp_path / "dev"), opts=opts)
    host = _run(exe, safe_case, str(tmp_path / "host"), opts=opts, env={"ITX_HOST_VETO": "1"})
    runs = ["host"]
    if os.path.exists(REF):
        _run(REF, safe_case, str(tmp_path / "ref"), opts=opts)
        runs.append("ref")
    names = sorted(fn for fn in os.listdir(tmp_path / "dev") if not fn.endswith(".bigWig"))
    assert len(names) == 6 + ("-B" in opts)
    for other in runs:
        for fn in names:
            assert filecmp.cmp(tmp_path / "dev" / fn, tmp_path / other / fn, shallow=False), (other, fn)
    n_dev, n_host = _routes(dev.stderr)
    assert n_dev >= 1 and n_host == 0, (n_dev, n_host)               # the device judged the batches
    assert _routes(host.stderr)[0] == 0
    _, tab = ac.table(ac.cases()[1])
    ext = 0 if "-E" in opts else 150
    safe = ac.subset(("ref_safe",))
    assert _vetoed(str(tmp_path / "dev")) == sum(bool(c and v) for c, v in (ac.verdict(r, tab, ac.cases()[1], ext) for r in safe)) > 500
