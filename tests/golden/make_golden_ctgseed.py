"""Writes tests/golden/ctg_s/: what the reference's own seeding (MaximalExactMatchWorkData_Init / _FindCandidates with extend_ctg_m4s' constants) answers on
  * craft.bin.gz     the crafted set of tests/ctg_seed_cases.py (seed 20261): contigs, reads, segments, jobs and answers in one case file;
  * nat.ans.bin.gz   the natural case: the committed contig and reads of tests/golden/ctg_g/nat*.bin.gz, every read a job on both strands - the answers alone.
The reference is compiled from its sources where they lie into a temporary directory (tests/golden/ctg_seed_ref_harness.c is our main around it); only data is
written here.  usage: python tests/golden/make_golden_ctgseed.py"""
import gzip
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from tests import ctg_seed_cases as sc      # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "ctg_s")
MAX_BYTES = 181770                           # the largest fixture committed before these
CRAFT_SEED = 20261


def _gz(src, dst):
    with open(src, "rb") as f, gzip.GzipFile(dst, "wb", 9, mtime=0) as g:
        g.write(f.read())
    assert os.path.getsize(dst) <= MAX_BYTES, (dst, os.path.getsize(dst))
    print(dst, os.path.getsize(dst), "bytes")


def main():
    assert sc.have_reference(), "the reference's sources are needed"
    os.makedirs(OUT, exist_ok=True)
    with tempfile.TemporaryDirectory() as tmp:
        exe = sc.build_harness(os.path.join(tmp, "harness"))
        cs = sc.crafted(CRAFT_SEED)
        sc.run_harness(exe, cs, tmp)
        sc.write_cases(cs, os.path.join(tmp, "craft.bin"))
        _gz(os.path.join(tmp, "craft.bin"), os.path.join(OUT, "craft.bin.gz"))
        nat = sc.natural()
        sc.run_harness(exe, nat, tmp)
        sc.write_answers(nat, os.path.join(tmp, "nat.ans.bin"))
        _gz(os.path.join(tmp, "nat.ans.bin"), os.path.join(OUT, "nat.ans.bin.gz"))
        for name, s in (("crafted", cs), ("natural", nat)):
            print(name, "segments", len(s.segments), "jobs", s.n_jobs(), "found", sum(a[0]["found"] for g in s.segments for a in g.answers),
                  "largest match list", max(a[1].shape[0] for g in s.segments for a in g.answers))


if __name__ == "__main__":
    main()
