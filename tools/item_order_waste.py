#!/usr/bin/env python3
"""The table of DESIGN 5.1: lane-steps the consumers of a round's ragged blocks issue against those the blocks need, in arrival order and in size-class
order, replayed on the CPU (tests/host_core/item_order_waste.cpp) on a synthetic read set with the bench's options at a reduced genome.  No GPU.

    python tools/item_order_waste.py [--genome 300000] [--coverage 40] [--seed 7]
"""
import argparse
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genome", type=int, default=300_000)
    ap.add_argument("--coverage", type=float, default=40.0)
    ap.add_argument("--seed", type=int, default=7)
    args = ap.parse_args()
    from necat_amd import synth
    with tempfile.TemporaryDirectory() as tmp:
        rs = synth.simulate_reads(args.genome, args.coverage, seed=args.seed)          # bench.py's read set at a smaller genome
        d = os.path.join(tmp, "vols")
        nv = synth.write_volume_dir(d, rs)
        assert nv == 1
        obj, exe = os.path.join(tmp, "necat_oracle.o"), os.path.join(tmp, "item_order_waste")
        subprocess.run(["gcc", "-O2", "-std=gnu99", "-c", os.path.join(ROOT, "oracle", "necat_oracle.c"), "-o", obj], check=True)
        subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-o", exe, os.path.join(ROOT, "tests", "host_core", "item_order_waste.cpp"), obj, "-lm", "-lpthread"], check=True)
        print("%d reads, %d bases; -k 15 -z 20 -q 500 -b 2000 -s 3 -n 500 -a 1000 -e 0.5 (bench.py's FAST)" % (rs.nreads, rs.nbases), flush=True)
        subprocess.run([exe, d, "0", "15", "20", "500", "2000", "3", "500", "1000", "0.5"], check=True)


if __name__ == "__main__":
    main()
