"""The library's knobs have ONE declaration - the table in necat_amd/csrc/knobs.h - and everything else that names a knob is checked against it here (no GPU)."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "necat_amd", "csrc")

# NUM(field, type, "NAME", default, min, max) | INT(field, "NAME", default) | SET(field, "NAME") | STR(field, "NAME")
LINE = re.compile(r'^\s*(NUM|INT|SET|STR)\(\s*(\w+)\s*,(?:\s*(\w+)\s*,)?\s*"(NECAT_[A-Z0-9_]+)"\s*(?:,\s*([^,)]+?)\s*)?[,)]', re.M)

# what the documents may name besides the table: the command-line programs' own variables (read by a process at its start: *_main.cpp, pm_job.h, asm_job.h),
# the tests' / bench's, and names that are no environment variables at all
PROGRAMS = {"NECAT_GPU", "NECAT_GPUS", "NECAT_PM_SCHEDULE", "NECAT_PM_PARTITIONS", "NECAT_PAIR_LANES", "NECAT_CLI_TRACE", "NECAT_CNS_PIPELINE", "NECAT_MKDB_GPU",
            "NECAT_MKDB_VOLSIZE", "NECAT_PM4_CHUNK", "NECAT_TRIM_HOST", "NECAT_ASM_CALL_ANCHORS", "NECAT_HIP_LIB", "NECAT_BENCH_ONE_DEVICE"}
EXPERIMENTS = {"NECAT_DEFER"}          # the knob of an experiment DESIGN.md reports and the tree never had (tools/r06/defer_experiment.patch)
NOT_VARIABLES = re.compile(r"NECAT_(ERR_[A-Z]+|OK|ABI_VERSION|BUILD_CROSSCHECK|XCHECK|TRIM_(NONE|COMPLETE|CHIMERIC|COVER)|HIP_H|RETIRED|HIP|CHECK_LAUNCH)$")


def _read(*p):
    with open(os.path.join(*p), encoding="utf-8") as f:
        return f.read()


def _table():
    return [m.groups() for m in LINE.finditer(_read(CSRC, "knobs.h"))]


def _per_call():
    """the variables knobs.h reads itself, per call (an entry point without a context)"""
    return set(re.findall(r'getenv\("(NECAT_[A-Z0-9_]+)"\)', _read(CSRC, "knobs.h")))


def _library_sources():
    """necat_hip.hip and every file of csrc it includes, directly or not"""
    seen, todo = set(), ["necat_hip.hip"]
    while todo:
        f = todo.pop()
        if f in seen or not os.path.exists(os.path.join(CSRC, f)):
            continue
        seen.add(f)
        todo += re.findall(r'^\s*#\s*include\s+"([^"/]+)"', _read(CSRC, f), re.M)
    return seen


def test_the_table_parses_and_names_nothing_twice():
    t = _table()
    text = _read(CSRC, "knobs.h")
    assert t and len(t) == len(re.findall(r"^\s*(?:NUM|INT|SET|STR)\(", text, re.M))          # every line of the list is understood
    fields, names = [r[1] for r in t], [r[3] for r in t]
    assert len(set(fields)) == len(fields), sorted(f for f in fields if fields.count(f) > 1)
    assert len(set(names)) == len(names), sorted(n for n in names if names.count(n) > 1)
    assert not _per_call() & set(names)
    assert _per_call() == {"NECAT_XGMI_GBS", "NECAT_INDEX_SHARD"}


def test_the_library_reads_its_environment_in_knobs_h_only():
    src = _library_sources()
    assert {"necat_hip.hip", "knobs.h", "runtime.h", "cns_loop.h", "stage_extend.inl", "stage_index.inl"} <= src, sorted(src)
    stage = {f for f in os.listdir(CSRC) if f.startswith("stage_") and f.endswith(".inl")}
    assert stage <= src, sorted(stage - src)
    for f in sorted(src - {"knobs.h"}):
        hits = [ln for ln in _read(CSRC, f).splitlines() if 'getenv("NECAT_' in ln]
        assert not hits, (f, hits)


def test_the_documents_and_the_table_name_the_same_knobs():
    docs = _read(ROOT, "INTEGRATION.md") + _read(ROOT, "DESIGN.md")
    mentioned = set(re.findall(r"NECAT_[A-Z0-9_]*[A-Z0-9]", docs))
    known = {r[3] for r in _table()} | _per_call()
    assert not known - mentioned, "knobs no document mentions: %s" % sorted(known - mentioned)
    stray = {n for n in mentioned - known - PROGRAMS - EXPERIMENTS if not NOT_VARIABLES.match(n)}
    assert not stray, "NECAT_* names of the documents that are no knob of knobs.h's table: %s" % sorted(stray)


def test_the_defaults_capi_restates_are_the_tables():
    from necat_amd import capi
    dflt = {r[3]: r[4] for r in _table() if r[0] in ("NUM", "INT")}
    for name, v in capi.XCHECK_DEFAULTS.items():
        assert name in dflt, name
        assert eval(dflt[name].replace("ull", "").replace("u", ""), {"__builtins__": {}}) == v, (name, dflt[name], v)
