#!/usr/bin/env python3
"""Scratch A/B of the whole command on one box: python tools/ab_cli.py <n_reads> <seq_len> <reps> NAME:VAR=VAL,VAR=VAL ...
Generates the bench inputs once (bench.py's generator), then runs `iteres stat -w` <reps> times per setting, interleaved.
LD_LIBRARY_PATH in a setting selects another build of libiteres_amd.so (the program's RUNPATH comes after it); ITX_AB_TREE=<dir below
the repository> runs the program of another built tree, which finds its own library (parent:ITX_AB_TREE=<an export of the parent commit>).
ITX_AB_FILTER=1 runs `iteres filter -c <the table's biggest class>` instead (ITX_AB_OPTS="-r": with the read lists) and compares
the .loci / .reportloci files; ITX_AB_SHUFFLED=1 runs every setting on reads_shuffled.bam, the same reads with mkbam's
order=shuffled (runs of 65 536 reads in a seeded random order, generated once beside reads.bam) (a setting may carry options of its own: `b:ITX_AB_OPTS=-b` is `filter -b` against plain `filter`); ITX_AB_FILTER=all runs `iteres filter` without a name filter (every row of the table is a line)."""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


class A:
    pass


def main():
    a = A()
    a.reads, a.seq_len, reps = int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3])
    a.rows, a.cpu_reads, a.workdir = 5_500_000, 0, ""
    # ITX_AB_MKBAM="content=hiseq cigar=mixed paired=1 pileup=20": what the BAM looks like (default: round 2's legacy content)
    for kv in os.environ.get("ITX_AB_MKBAM", "").split():
        k, v = kv.split("=", 1)
        setattr(a, k, int(v) if v.isdigit() else v)
    wd, info = bench.ensure_inputs(a, 16)
    reads = os.path.join(wd, "reads.bam")
    if os.environ.get("ITX_AB_SHUFFLED"):
        reads = os.path.join(wd, "reads_shuffled.bam")
        if not os.path.exists(reads):
            subprocess.check_call([bench.MKBAM, os.path.join(wd, "chrom.sizes"), str(a.reads), reads + ".tmp", str(a.seq_len), "7"] + bench.mkbam_options(a) + ["order=shuffled"],
                                  env=dict(os.environ, OMP_NUM_THREADS="16"))
            os.rename(reads + ".tmp", reads)
    settings = [("base", {})]
    for spec in sys.argv[4:]:
        name, kv = spec.split(":", 1)
        settings.append((name, dict(x.split("=", 1) for x in kv.split(",") if x)))
    walls = {n: [] for n, _ in settings}
    scans = {n: [] for n, _ in settings}
    notes = {}
    for rep in range(reps):
        for name, kv in settings:
            env = dict(os.environ, OMP_NUM_THREADS="16", ITX_TIMING="1", ITX_GPUS="1")
            for k, v in kv.items():
                env[k] = os.path.join(ROOT, v) if k == "LD_LIBRARY_PATH" else v
            out = os.path.join(wd, "ab_" + name)
            args = bench.base_args(wd)
            extra = env.get("ITX_AB_OPTS", "").split()                     # e.g. ITX_AB_OPTS="-R": options behind `stat -w`; inside a setting (b:ITX_AB_OPTS=-b): for that setting alone
            args = args[:2] + extra + args[2:]
            if os.environ.get("ITX_AB_FILTER"):
                select = [] if os.environ["ITX_AB_FILTER"] == "all" else ["-c", info["filter_class"]["name"]]
                args = ["filter"] + select + extra + args[2:]
            exe = os.path.join(ROOT, kv["ITX_AB_TREE"], "iteres_amd", "host", "iteres") if "ITX_AB_TREE" in kv else bench.OURS     # parent:ITX_AB_TREE=<dir>: the program (and library) of another built tree
            wall, rc, err, seen = bench.run_timed(exe, args + [reads], out, env, (bench.SCAN_BEGIN, bench.SCAN_END))
            assert rc == 0, err[-800:]
            walls[name].append(round(wall, 3))
            scans[name].append(round(seen.get(bench.SCAN_END, 0) - seen.get(bench.SCAN_BEGIN, 0), 3))
            notes[name] = [ln[13:] for ln in err.replace("\r", "\n").split("\n") if ln.startswith("[itx timing]")]
    same = {}
    for name, _ in settings[1:]:
        outputs = bench.TEXT_OUTPUTS
        if os.environ.get("ITX_AB_FILTER"):
            outputs = sorted(fn for fn in os.listdir(os.path.join(wd, "ab_base")) if fn.endswith("loci"))
            assert len(outputs) == 2, outputs
        same[name] = all(open(os.path.join(wd, "ab_base", fn), "rb").read() == open(os.path.join(wd, "ab_" + name, fn), "rb").read() for fn in outputs)
    print(json.dumps({"reads": a.reads, "seq_len": a.seq_len, "walls_s": walls, "scan_s": scans, "same_outputs_as_base": same, "notes": notes, "inputs": info}), flush=True)


if __name__ == "__main__":
    main()
