"""The environment switches (mauvealigner_amd/csrc/switches.hpp): the table as a fresh process fills it from a given environment
(tests/cpp/switches_test.cpp, host C++ only) against the values written out here -- every default and every parse rule that is not
"present = on" -- and, by reading files: the table is the only place in csrc that reads the environment, INTEGRATION.md lists the
table's switches with their kinds, and the switches that were removed stay out of csrc."""
import glob
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mauvealigner_amd", "csrc")
TABLE = os.path.join(CSRC, "switches.hpp")

# nothing set.  0 for MAUVE_SCHEDULE, MAUVE_HOST_THREADS and MAUVE_CH_CL_MAX is "not set": the runtime's wait, one thread (workers.hpp)
# and CH_CL_MAX (chain_dev.hip) are chosen where the field is read
DEFAULTS = {
    "MAUVE_TRACE": 0, "MAUVE_SCHEDULE": 0, "MAUVE_HOST_THREADS": 0, "MAUVE_SMALL_SORT": 1, "MAUVE_WIDE_INDEX": 0, "MAUVE_NO_TINY": 0,
    "MAUVE_RUNS_ITEMS": 0, "MAUVE_LIST_CAP": 0, "MAUVE_CANON_DEVICE_MIN": 16384, "MAUVE_CH_BIG_MAX": 2048, "MAUVE_CH_CL_MAX": 0,
    "MAUVE_HOST_CHAIN": 0, "MAUVE_HOST_TAIL": 0, "MAUVE_HOST_EXTEND": 0, "MAUVE_EXT_DECLINE": 0, "MAUVE_GIVEN_ON_HOST": 0,
    "MAUVE_HOST_GAP_CHAIN": 0, "MAUVE_GAP_CHAIN_ALL_BACK": 0, "MAUVE_SHARD_SINGLE": 0, "MAUVE_BB_COLUMN_SCAN": 0, "MAUVE_DP_CLASS": 0,
    "MAUVE_DP_WIDE_MIN": 1024, "MAUVE_DP_BIG_MAX": 256, "MAUVE_DP_CLUSTER": 32, "MAUVE_DP_DESC_MIN": 2048, "MAUVE_DP_TB_BUDGET": 8 << 30,
    "MAUVE_DP_NO_WIDE": 0, "MAUVE_DP_NOSCAN": 0, "MAUVE_DP_ONE_WAVE": 0, "MAUVE_DP_NO_GROUPS": 0, "MAUVE_DP_DESC_HOST": 0,
}
# the switches whose rule is "present, even with an empty value = on"
FLAGS = ("MAUVE_TRACE", "MAUVE_NO_TINY", "MAUVE_HOST_CHAIN", "MAUVE_HOST_TAIL", "MAUVE_HOST_EXTEND", "MAUVE_EXT_DECLINE", "MAUVE_GIVEN_ON_HOST",
         "MAUVE_HOST_GAP_CHAIN", "MAUVE_GAP_CHAIN_ALL_BACK", "MAUVE_SHARD_SINGLE", "MAUVE_BB_COLUMN_SCAN", "MAUVE_DP_NO_WIDE", "MAUVE_DP_NOSCAN",
         "MAUVE_DP_ONE_WAVE", "MAUVE_DP_NO_GROUPS", "MAUVE_DP_DESC_HOST")
REMOVED = ("MAUVE_ELIM_COMPACT", "MAUVE_NO_SHADOW", "MAUVE_NO_KEEP_MUMS", "MAUVE_HOST_DP_FRONT", "MAUVE_TRACE_MATCHES")
KIND_WORDS = {"DIAGNOSTIC": "diagnostic", "TEST_KNOB": "test knob", "AB": "A/B", "OPERATIONAL": "operational"}

# (name, value in the environment, value in the table)
RULES = [
    ("MAUVE_SMALL_SORT", "0", 0), ("MAUVE_SMALL_SORT", "00", 0), ("MAUVE_SMALL_SORT", "1", 1), ("MAUVE_SMALL_SORT", "", 1),
    ("MAUVE_WIDE_INDEX", "1", 1), ("MAUVE_WIDE_INDEX", "0", 0), ("MAUVE_WIDE_INDEX", "11", 0),
    ("MAUVE_RUNS_ITEMS", "8", 8), ("MAUVE_RUNS_ITEMS", "5", 0),
    ("MAUVE_CH_BIG_MAX", "0", 1), ("MAUVE_DP_TB_BUDGET", "1", 65536), ("MAUVE_HOST_THREADS", "0", 1), ("MAUVE_HOST_THREADS", "99", 16),
    ("MAUVE_DP_CLASS", "bound", 1), ("MAUVE_DP_CLASS", "wild", 2), ("MAUVE_DP_CLASS", "x", 0),
    # the remaining rows of the rule table: plain numbers, the lower end of MAUVE_CH_CL_MAX, the three schedules
    ("MAUVE_LIST_CAP", "100", 100), ("MAUVE_CANON_DEVICE_MIN", "1", 1), ("MAUVE_CH_BIG_MAX", "7", 7), ("MAUVE_CH_CL_MAX", "0", 1),
    ("MAUVE_CH_CL_MAX", "8", 8), ("MAUVE_DP_WIDE_MIN", "0", 0), ("MAUVE_DP_BIG_MAX", "2", 2), ("MAUVE_DP_CLUSTER", "0", 0),
    ("MAUVE_DP_DESC_MIN", "1", 1), ("MAUVE_DP_TB_BUDGET", "1000000", 1000000), ("MAUVE_HOST_THREADS", "4", 4),
    ("MAUVE_SCHEDULE", "spin", 1), ("MAUVE_SCHEDULE", "yield", 2), ("MAUVE_SCHEDULE", "block", 3),
] + [(name, "", 1) for name in FLAGS]


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("switches") / "switches_test")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I" + CSRC, os.path.join(ROOT, "tests", "cpp", "switches_test.cpp"), "-o", path])
    return path


def table_of(exe, env):
    """the table of a fresh process whose only MAUVE_* variables are env's"""
    full = {k: v for k, v in os.environ.items() if not k.startswith("MAUVE_")}
    full.update(env)
    out = subprocess.run([exe], env=full, capture_output=True, text=True, check=True).stdout
    pairs = [line.split("=") for line in out.splitlines()]
    assert len(pairs) == len({n for n, _ in pairs}), "a name appears twice in the table"
    return {n: int(v) for n, v in pairs}


def test_defaults(exe):
    assert table_of(exe, {}) == DEFAULTS


@pytest.mark.parametrize("name,value,want", RULES, ids=["%s=%s" % (n, v) for n, v, _ in RULES])
def test_parse_rule(exe, name, value, want):
    assert table_of(exe, {name: value}) == dict(DEFAULTS, **{name: want})       # (and no other field moves)


def _table_lines():
    with open(TABLE) as f:
        return re.findall(r'^\s*X\(\s*\w+,\s*\w+,\s*"(MAUVE_\w+)",\s*(\w+),', f.read(), re.M)


def test_the_table_is_the_only_reader_of_the_environment():
    assert set(n for n, _ in _table_lines()) == set(DEFAULTS)
    for path in sorted(glob.glob(os.path.join(CSRC, "*"))):
        if os.path.isfile(path) and path != TABLE and not path.endswith((".o", ".so")):
            with open(path, errors="replace") as f:
                assert "getenv(" not in f.read(), path


def test_integration_md_lists_the_table():
    with open(os.path.join(ROOT, "INTEGRATION.md")) as f:
        text = f.read()
    section = re.search(r"^## Environment switches\n(.*?)(?=^## |\Z)", text, re.M | re.S)
    assert section, "INTEGRATION.md has no section 'Environment switches'"
    rows = re.findall(r"^\| `(MAUVE_\w+)` \|[^|]*\|[^|]*\| ([^|]*?) \|", section.group(1), re.M)
    assert rows == [(n, KIND_WORDS[k]) for n, k in _table_lines()]               # the same switches, in the table's order, with their kinds
    assert "before the first context is created" in section.group(1)


def test_removed_switches_stay_out_of_csrc():
    for path in sorted(glob.glob(os.path.join(CSRC, "*"))):
        if os.path.isfile(path) and not path.endswith((".o", ".so")):
            with open(path, errors="replace") as f:
                text = f.read()
            for name in REMOVED:
                assert name not in text, (path, name)
