"""The cases of the bigWig build of `filter -W` at the C ABI (tests/test_gpu_gcov_bigwig.py), as intervals that go into the
coverage, with what each is there for. `all_cases()` gives, per case, the chromosome sizes and the bedGraph items of both files
(all intervals; those marked unique) as the depth of the intervals: what tests/bwsparse.py model() and the reference's converter
take. tests/test_gcov_bigwig_cases.py checks on the CPU that every case has the property it is named for.

A case is (chroms, intervals): chroms [(name, size)] in the size file's order, intervals [(name, start, end, unique)] with
0 <= start < end <= size - 1 (what the coverage accepts)."""
import numpy as np

import bwsparse as bs


def _case_sections():
    """section boundaries: chromosomes with 1023, 1024, 1025 and 2049 items, one with a single item, one without data between two
    with data; chr1 < chr10 < chr2 in byte order whatever the file order"""
    chroms = [("chr2", 20000), ("chr1", 20000), ("chr10", 20000), ("chr3", 30000), ("chr4", 5000), ("chr5", 5000)]
    iv = []
    for name, k in (("chr1", 1023), ("chr10", 1024), ("chr2", 1025), ("chr3", 2049)):
        iv += [(name, s, e, i % 3 != 0) for i, (s, e) in enumerate(bs.exact_items(k, 7 + len(name)))]
    iv.append(("chr5", 4000, 4100, True))
    return chroms, iv


def chain_layout(R):
    """the engineered chromosome for a first reduction R: (intervals, size, marks). Groups lie 8 R apart (a definite re-anchor); where
    a group starts with an anchor item [a, a + 5), that item's summary ends at E = a + R. marks name the item starts the tests look
    for."""
    iv, marks, at = [], {}, [1000]

    def group():
        at[0] += 8 * R
        return at[0]
    for name, g in (("gap_R-1", R - 1), ("gap_R", R), ("gap_2R-2", 2 * R - 2), ("gap_2R-1", 2 * R - 1)):
        a = group()                                        # the second item starts g behind the open summary's end
        iv += [(a, a + 5), (a + R + g, a + R + g + 5)]
        marks[name] = a + R + g
    G = 2 * R - 6                                          # one gap between neighbours, two phases
    a = group()
    iv += [(a, a + 5), (a + 5 + G, a + 10 + G)]            # R - 1 behind E: goes on at E
    marks["amb_stays"] = a + 5 + G
    a = group()                                            # the item before the gap ends one base before E: 2 R - 7 behind E, re-anchors
    iv += [(a, a + 5), (a + R - 6, a + R - 1), (a + R - 1 + G, a + R + 4 + G)]
    marks["amb_anchors"] = a + R - 1 + G
    a = group()                                            # two ambiguous gaps in a row
    iv += [(a, a + 5), (a + 5 + R + 3, a + 10 + R + 3), (a + 10 + 2 * (R + 3), a + 15 + 2 * (R + 3))]
    marks["amb_twice"] = a + 10 + 2 * (R + 3)
    a = group()                                            # one item over four summaries
    iv.append((a, a + 3 * R + 7))
    marks["long"] = a
    a = group()                                            # 120 items of one base inside one summary
    iv += [(a + 2 * i, a + 2 * i + 1) for i in range(120)]
    marks["many"] = a
    size = at[0] + 8 * R + 43
    iv.append((size - 41, size - 1))                       # ends at size - 1; its summary is clipped to the size
    marks["clipped"] = size - 41
    return iv, size, marks


def _case_chain():
    """the chain's decisions. The bulk on chrB (items of 30 bases, 30 apart) sets the reduction; chrG is laid out for that reduction,
    which in turn depends a little on chrG: iterated to a fixed point, and the test asserts the model's first reduction is the R used"""
    bulk = [("chrB", s, e, True) for s, e in bs.exact_items(3000, 100, 30, 30)]
    R = 300
    for _ in range(20):
        iv, size, marks = chain_layout(R)
        chroms = [("chrB", 200000), ("chrG", size)]
        case = chroms, bulk + [("chrG", s, e, i % 2 == 0) for i, (s, e) in enumerate(iv)]
        got = bs.model(items_of_case(case)[0], dict(chroms))["zooms"][0][0]
        if got == R:
            return case
        R = got
    raise AssertionError("the chain case found no fixed point")


def _case_loop():
    """the first-reduction loop goes round: tries = 1 + rounds (the seed is pinned by tests/test_gcov_bigwig_cases.py)"""
    rng = np.random.default_rng(11)
    chroms = [("chrA", 400000), ("chrC", 400000)]
    iv = [("chrA", s, e, bool(rng.integers(0, 2))) for s, e in bs.blocks(rng, 700, 50, 30, end_before=399000)]
    iv += [("chrC", s, e, bool(rng.integers(0, 2))) for s, e in bs.blocks(rng, 300, 90, 900, end_before=399000)]
    return chroms, iv


def _case_twoblocks():
    """more than 1024 summaries at the first level: two zoom blocks"""
    chroms = [("chr7", 100000)]
    return chroms, [("chr7", s, e, i % 4 == 0) for i, (s, e) in enumerate(bs.exact_items(30000, 11, 1, 2))]


def _case_uniq_empty():
    """no interval is unique: the second file has no data while the first has"""
    chroms = [("chr1", 50000), ("chr2", 50000)]
    rng = np.random.default_rng(5)
    return chroms, [("chr2", s, e, False) for s, e in bs.blocks(rng, 300, 10, 60, end_before=49000)]


CASES = {"sections": _case_sections, "chain": _case_chain, "loop": _case_loop, "twoblocks": _case_twoblocks, "uniq_empty": _case_uniq_empty}
_made = {}


def case(key):
    if key not in _made:
        _made[key] = CASES[key]()
    return _made[key]


def items_of_case(c):
    """-> [items of all intervals, items of the unique ones], each {name: [(start, end, depth)]}"""
    chroms, iv = c
    out = []
    for only_unique in (False, True):
        by = {}
        for name, s, e, u in iv:
            if u or not only_unique:
                by.setdefault(name, []).append((s, e))
        out.append({n: bs.depth_items(v) for n, v in by.items()})
    return out


def all_cases():
    return {k: (dict(case(k)[0]), items_of_case(case(k))) for k in CASES}
