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
spread (max - min) of either set, in the device's favour.

    python tools/sam_ab.py --bgzf [reads=50000000] [--out profiles/r13_cli_samgz_device_vs_host.json]

writes the same SAM as BGZF (members of 0xff00 bytes, the EOF marker) next to the text and times `stat -w -S` and `stat -w -S -x` on it
by three routes: inflated and parsed on the device (ITX_HOST_SAM=0), inflated by the host and parsed on the device
(ITX_HOST_SAM=0 ITX_HOST_SAM_INFLATE=1), and the host's reader (ITX_HOST_SAM=1); plain-text -S under ITX_HOST_SAM=0 on the same reads is
the yardstick beside them. Interleaved, --runs runs each, all outputs compared byte for byte; the same rule, device inflate against
each of the two host routes."""
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
import zlib

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


def run(exe, d, out, opts, route, aln="reads.sam", env=None):
    shutil.rmtree(out, ignore_errors=True)
    os.makedirs(out)
    cmd = [exe, "stat", "-S"] + opts + ["-o", "out", os.path.join(d, "chrom.sizes"), os.path.join(d, "rep.sizes"), os.path.join(d, "rmsk.txt"), os.path.join(d, aln)]
    t0 = time.perf_counter()
    base = {k: v for k, v in os.environ.items() if k != "ITX_HOST_SAM_INFLATE"}
    pr = subprocess.run(cmd, cwd=out, capture_output=True, text=True, env=dict(base, ITX_TIMING="1", ITX_HOST_SAM=route, **(env or {})))
    wall = time.perf_counter() - t0
    if pr.returncode != 0:
        raise SystemExit(f"{' '.join(cmd)} failed ({pr.returncode}):\n{pr.stderr[-2000:]}")
    keep = ("[itx timing] sam:", "[itx timing] sam gz:", "[itx timing] stream of", "[itx timing] open")
    return wall, [l for l in pr.stderr.replace("\r", "\n").split("\n") if l.startswith(keep)]


BGZF_EOF = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


def write_bgzf(src, dst, payload=0xff00, level=6):
    """src as a chain of BGZF members of `payload` bytes and the EOF marker (what bgzip writes)"""
    with open(src, "rb") as f, open(dst, "wb") as g:
        while True:
            data = f.read(payload)
            if not data:
                break
            co = zlib.compressobj(level, zlib.DEFLATED, -15)
            comp = co.compress(data) + co.flush()
            g.write(b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff\x06\x00BC\x02\x00" + (len(comp) + 25).to_bytes(2, "little") + comp
                    + (zlib.crc32(data) & 0xFFFFFFFF).to_bytes(4, "little") + len(data).to_bytes(4, "little"))
        g.write(BGZF_EOF)


def same_outputs(a, b):
    names = sorted(os.listdir(a))
    return names == sorted(os.listdir(b)) and all(filecmp.cmp(os.path.join(a, f), os.path.join(b, f), shallow=False) for f in names)


def main_bgzf(a, exe, d, path, n, base_reads):
    gz = os.path.join(d, "reads.sam.gz")
    write_bgzf(path, gz)
    routes = {"device_inflate": ("0", "reads.sam.gz", {}), "host_inflate_device_parse": ("0", "reads.sam.gz", {"ITX_HOST_SAM_INFLATE": "1"}),
              "host": ("1", "reads.sam.gz", {}), "plain_text_device_parse": ("0", "reads.sam", {})}
    result = {"reads": n, "base_reads": base_reads, "sam_bytes": os.path.getsize(path), "bgzf_bytes": os.path.getsize(gz),
              "chunk_bytes": os.environ.get("ITX_SAM_CHUNK", "default (64 MiB)"), "commands": []}
    for opts in (["-w"], ["-w", "-x"]):
        run(exe, d, os.path.join(d, "warm"), opts, "1", "reads.sam.gz")       # page cache and device warm, not counted
        run(exe, d, os.path.join(d, "warm"), opts, "1", "reads.sam")
        walls = {r: [] for r in routes}
        timing = {}
        for k in range(a.runs):
            for r, (route, aln, env) in routes.items():
                w, lines = run(exe, d, os.path.join(d, "out_" + r), opts, route, aln, env)
                walls[r].append(round(w, 3))
                timing[r] = lines
            for r in routes:
                if not same_outputs(os.path.join(d, "out_device_inflate"), os.path.join(d, "out_" + r)):
                    raise SystemExit(f"stat {' '.join(opts)}: the routes device_inflate and {r} wrote different files in {d}")
        med = {r: statistics.median(v) for r, v in walls.items()}
        spread = {r: round(max(v) - min(v), 3) for r, v in walls.items()}
        faster = {r: bool(med[r] - med["device_inflate"] > max(spread[r], spread["device_inflate"])) for r in ("host_inflate_device_parse", "host")}
        result["commands"].append({"opts": ["-S"] + opts, "wall_s": walls, "median_s": med, "spread_s": spread, "device_inflate_faster_by_the_rule_than": faster,
                                   "outputs_identical": True, "timing": timing})
        print(json.dumps(result["commands"][-1]), flush=True)
    result["device_inflate_pays"] = all(all(c["device_inflate_faster_by_the_rule_than"].values()) for c in result["commands"])
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(f"device inflate pays by the rule: {result['device_inflate_pays']} -> {a.out}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("reads", nargs="?", type=int, default=50_000_000)
    ap.add_argument("--base-reads", type=int, default=1_000_000)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--bgzf", action="store_true", help="the same SAM as BGZF: device inflate against the host's inflate and the host's reader")
    ap.add_argument("--out", default=None, help="default: profiles/r12_cli_sam_device_vs_host.json, with --bgzf profiles/r13_cli_samgz_device_vs_host.json")
    ap.add_argument("--keep", default=None, help="directory for the inputs (kept); default: a temporary one")
    a = ap.parse_args()
    if a.out is None:
        a.out = os.path.join(ROOT, "profiles", "r13_cli_samgz_device_vs_host.json" if a.bgzf else "r12_cli_sam_device_vs_host.json")
    _, exe = build.build_all()
    d = a.keep or tempfile.mkdtemp(prefix="itx_sam_ab_")
    os.makedirs(d, exist_ok=True)
    base_reads = min(a.base_reads, a.reads)
    path, n = make_inputs(d, a.reads, base_reads)
    if a.bgzf:
        main_bgzf(a, exe, d, path, n, base_reads)
        if not a.keep:
            shutil.rmtree(d, ignore_errors=True)
        return
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
