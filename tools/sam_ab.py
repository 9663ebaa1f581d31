#!/usr/bin/env python3
"""`iteres stat -S` with the SAM text parsed on the device (ITX_HOST_SAM=0, csrc/itx_samtext.hip) against the host's line
parser (ITX_HOST_SAM=1), interleaved, page cache warm.

    python tools/sam_ab.py [reads=50000000] [--base-reads 1000000] [--runs 3] [--out profiles/r12_cli_sam_device_vs_host.json] [--keep DIR]

1. a synthetic SAM of --base-reads reads (iteres_amd.synth.write_sam; every mapped read has a CIGAR, XA on a quarter of them),
2. its body repeated up to <reads> lines,
3. `stat -w -S` under ITX_HOST_SAM=0 and =1 in turn, --runs runs each, then the same for `stat -w -S -x`,
4. every output file of the two routes compared byte for byte,
5. the wall times, the medians and spreads, the ITX_TIMING lines and the verdict of the rule into --out.
The rule (the bed route's): the device route is the faster one for a command when the two medians differ by more than the
spread (max - min) of either set, in the device's favour."""
import argparse
import filecmp
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from iteres_amd import build, synth  # noqa: E402


def make_inputs(d, reads, base_reads):
    chroms = [("chr1", 120_000_000), ("chr2", 90_000_000), ("chr3", 50_000_000), ("chrM", 16_571)]
    t = synth.make_table(1201, chroms, 200_000, n_names=800, n_fams=40, n_clas=12, overlap_frac=0.02)
    synth.write_sizes(os.path.join(d, "chrom.sizes"), chroms)
    synth.write_sizes(os.path.join(d, "rep.sizes"), t.rep_len.items())
    synth.write_rmsk(os.path.join(d, "rmsk.txt"), t)
    r = synth.make_reads(1202, chroms, base_reads, read_len=(100, 100), paired_frac=0.0, nocigar_frac=0.0)
    rng = np.random.default_rng(1203)
    xa = rng.random(len(r)) < 0.25
    alt = rng.integers(1, 50_000_000, len(r))
    r.aux = [[f"NM:i:{i & 3}", f"XA:Z:chr{1 + (i % 3)},{'+-'[i & 1]}{int(alt[i])},100M,{i % 4};"] if xa[i] else [f"NM:i:{i & 1}"] for i in range(len(r))]
    base = os.path.join(d, "base.sam")
    synth.write_sam(base, r)
    text = open(base, "rb").read()
    cut = 0
    while text[cut:cut + 1] == b"@":
        cut = text.index(b"\n", cut) + 1
    header, body = text[:cut], text[cut:]
    path = os.path.join(d, "reads.sam")
    n = 0
    with open(path, "wb") as f:
        f.write(header)
        while n < reads:
            if reads - n >= base_reads:
                f.write(body)
                n += base_reads
            else:
                stop = 0
                for _ in range(reads - n):
                    stop = body.index(b"\n", stop) + 1
                f.write(body[:stop])
                n = reads
    os.unlink(base)
    return path, n


def run(exe, d, out, opts, route):
    shutil.rmtree(out, ignore_errors=True)
    os.makedirs(out)
    cmd = [exe, "stat", "-S"] + opts + ["-o", "out", os.path.join(d, "chrom.sizes"), os.path.join(d, "rep.sizes"), os.path.join(d, "rmsk.txt"), os.path.join(d, "reads.sam")]
    t0 = time.perf_counter()
    pr = subprocess.run(cmd, cwd=out, capture_output=True, text=True, env=dict(os.environ, ITX_TIMING="1", ITX_HOST_SAM=route))
    wall = time.perf_counter() - t0
    if pr.returncode != 0:
        raise SystemExit(f"{' '.join(cmd)} failed ({pr.returncode}):\n{pr.stderr[-2000:]}")
    keep = ("[itx timing] sam:", "[itx timing] stream of", "[itx timing] open")
    return wall, [l for l in pr.stderr.replace("\r", "\n").split("\n") if l.startswith(keep)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("reads", nargs="?", type=int, default=50_000_000)
    ap.add_argument("--base-reads", type=int, default=1_000_000)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r12_cli_sam_device_vs_host.json"))
    ap.add_argument("--keep", default=None, help="directory for the inputs (kept); default: a temporary one")
    a = ap.parse_args()
    _, exe = build.build_all()
    d = a.keep or tempfile.mkdtemp(prefix="itx_sam_ab_")
    os.makedirs(d, exist_ok=True)
    base_reads = min(a.base_reads, a.reads)
    path, n = make_inputs(d, a.reads, base_reads)
    result = {"reads": n, "base_reads": base_reads, "sam_bytes": os.path.getsize(path), "chunk_bytes": os.environ.get("ITX_SAM_CHUNK", "default (64 MiB)"), "commands": []}
    open(path, "rb").read(1 << 20)
    for opts in (["-w"], ["-w", "-x"]):
        run(exe, d, os.path.join(d, "warm"), opts, "1")                    # page cache and device warm, not counted
        walls = {"0": [], "1": []}
        timing = {}
        for k in range(a.runs):
            for route in ("0", "1"):
                w, lines = run(exe, d, os.path.join(d, f"out{route}"), opts, route)
                walls[route].append(round(w, 3))
                timing[route] = lines
            o0, o1 = os.path.join(d, "out0"), os.path.join(d, "out1")
            names = sorted(os.listdir(o0))
            if names != sorted(os.listdir(o1)) or not all(filecmp.cmp(os.path.join(o0, f), os.path.join(o1, f), shallow=False) for f in names):
                raise SystemExit(f"stat {' '.join(opts)}: the two routes wrote different files in {d}")
        med = {r: statistics.median(v) for r, v in walls.items()}
        spread = {r: max(v) - min(v) for r, v in walls.items()}
        faster = med["1"] - med["0"] > max(spread.values())
        result["commands"].append({"opts": ["-S"] + opts, "device_wall_s": walls["0"], "host_wall_s": walls["1"], "device_median_s": med["0"], "host_median_s": med["1"],
                                   "device_spread_s": round(spread["0"], 3), "host_spread_s": round(spread["1"], 3), "device_faster_by_the_rule": bool(faster),
                                   "outputs_identical": True, "device_timing": timing["0"], "host_timing": timing["1"]})
        print(json.dumps(result["commands"][-1]), flush=True)
    result["device_becomes_default"] = all(c["device_faster_by_the_rule"] for c in result["commands"])
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    if not a.keep:
        shutil.rmtree(d, ignore_errors=True)
    print(f"device route becomes the default: {result['device_becomes_default']} -> {a.out}")


if __name__ == "__main__":
    main()
