#!/usr/bin/env python3
"""What the levels of `filter -b -l` cost in size, on the CPU: python tools/levels_ratio.py [MiB of records, default 64]
tools/mkbam.c makes `hiseq` reads (100 bases + qualities, cigar=mixed); the first <MiB> MiB of their records are cut into payloads
of ITX_BAMOUT_PAYLOAD bytes, as the writer cuts them, and every payload goes through the host build of the member rule
(tests/bgzflevels_host.cpp) at levels 1 and 6 and through zlib's level 1 as a raw DEFLATE stream of its own. Prints one JSON line:
the three totals (levels 1 and 6: whole members, 26 bytes of frame each; zlib: the DEFLATE bytes plus the same 26) and the quotients."""
import json
import os
import subprocess
import sys
import tempfile
import zlib
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import bgzflevelshost as bl  # noqa: E402
import refio  # noqa: E402
from iteres_amd import synth  # noqa: E402


def main():
    mib = int(sys.argv[1]) if len(sys.argv) > 1 else 64
    want = mib << 20
    with tempfile.TemporaryDirectory() as d:
        mkbam = os.path.join(d, "mkbam")
        subprocess.check_call(["gcc", "-O2", "-fopenmp", "-o", mkbam, os.path.join(ROOT, "tools", "mkbam.c"), "-lz", "-ldl"])
        synth.write_sizes(os.path.join(d, "chrom.sizes"), synth.HG38_CHROMS)
        n_reads = want // 200 + 10_000                                     # a record of these reads is ~220 bytes
        subprocess.check_call([mkbam, os.path.join(d, "chrom.sizes"), str(n_reads), os.path.join(d, "reads.bam"), "100", "7", "content=hiseq", "cigar=mixed"])
        raw = refio.bgzf_decompress(open(os.path.join(d, "reads.bam"), "rb").read())
        rule = bl.LevelRule(d)
        # the records behind the header
        l_text = int.from_bytes(raw[4:8], "little")
        at = 8 + l_text
        n_ref = int.from_bytes(raw[at:at + 4], "little")
        at += 4
        for _ in range(n_ref):
            at += 8 + int.from_bytes(raw[at:at + 4], "little")
        data = raw[at:at + want]
        assert len(data) == want, "too few reads"
        P = rule.payload
        slices = [data[i:i + P] for i in range(0, len(data), P)]

        def one(b):
            z = zlib.compressobj(1, zlib.DEFLATED, -15)
            return len(rule.member(b, 1)), len(rule.member(b, 6)), len(z.compress(b) + z.flush()) + 26
        with ThreadPoolExecutor(max(os.cpu_count() or 1, 1)) as ex:         # (ctypes calls release the GIL)
            res = list(ex.map(one, slices, chunksize=64))
    t1, t6, tz = (sum(r[k] for r in res) for k in range(3))
    print(json.dumps({"what": f"{mib} MiB of hiseq BAM records (tools/mkbam.c content=hiseq cigar=mixed, 100 bases) in {len(slices)} payloads of {P} bytes",
                      "payload_bytes": len(data), "level_1_bytes": t1, "level_6_bytes": t6, "zlib_1_bytes": tz,
                      "level_1_over_level_6": round(t1 / t6, 4), "level_1_over_zlib_1": round(t1 / tz, 4),
                      "level_1_over_payload": round(t1 / len(data), 4), "level_6_over_payload": round(t6 / len(data), 4)}))


if __name__ == "__main__":
    main()
