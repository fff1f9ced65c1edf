// switches.hpp -- every environment switch of libmauve_hip.so: one table, filled once per process.
//
// switches() reads the environment the first time it is called, which is when the first context is created
// (mauve_ctx_create), so a switch is set before that; nothing on a timed path reads the environment.  This is the only
// file of csrc that calls getenv.  A switch is its line in MAUVE_SWITCHES plus the site that reads its field;
// INTEGRATION.md ("Environment switches") lists the same names for users, and tests/test_switches_cpu.py holds the
// two lists and the parse rules below to each other.  Plain C++17: no HIP, no common.hpp (host tests build it with g++).
//
// Kinds:  DIAGNOSTIC   prints; changes no result
//         TEST_KNOB    lowers a limit so that small inputs reach an edge
//         AB           forces a path that the code otherwise selects by itself
//         OPERATIONAL  a setting for deployments: the only kind that is part of the supported interface
#pragma once
#include <cstdint>
#include <cstdlib>
#include <cstring>

inline long long sw_at_least(long long v, long long lo) { return v < lo ? lo : v; }
inline long long sw_within(long long v, long long lo, long long hi) { return v < lo ? lo : v > hi ? hi : v; }
inline int sw_run_items(int v) { return v == 4 || v == 8 || v == 16 ? v : 0; }

// X(type, field, "NAME", kind, the field's value from e = getenv("NAME") (null when unset), "what it does")
#define MAUVE_SWITCHES(X) \
    X(bool,     trace,              "MAUVE_TRACE",              DIAGNOSTIC,  e != nullptr, "[trace] lines on stderr: stage times, counts and the path each stage took") \
    X(int,      schedule,           "MAUVE_SCHEDULE",           OPERATIONAL, !e ? 0 : !strcmp(e, "spin") ? 1 : !strcmp(e, "yield") ? 2 : 3, "how the host waits for the device: spin (1), yield (2), anything else block (3); unset (0) leaves the runtime's choice") \
    X(int,      host_threads,       "MAUVE_HOST_THREADS",       OPERATIONAL, !e ? 0 : sw_within(atoi(e), 1, 16), "host threads of the assembly loops, 1..16; unset (0): the rule in workers.hpp") \
    X(bool,     small_sort,         "MAUVE_SMALL_SORT",         AB,          !(e && e[0] == '0'), "a value starting with 0 sends sorts of up to SS_CAP pairs through the tiled radix sort too") \
    X(bool,     wide_index,         "MAUVE_WIDE_INDEX",         AB,          e && e[0] == '1' && e[1] == 0, "exactly 1: every seed pass takes the 64-bit window index, not only those of 2^31 windows or more") \
    X(bool,     no_tiny,            "MAUVE_NO_TINY",            AB,          e != nullptr, "a seed pass of a few thousand windows takes the hash join like any other") \
    X(int,      runs_items,         "MAUVE_RUNS_ITEMS",         AB,          sw_run_items(e ? atoi(e) : 0), "4, 8 or 16: that run-tile instantiation for every launch; else 0, chosen by launch size") \
    X(uint32_t, list_cap,           "MAUVE_LIST_CAP",           TEST_KNOB,   e ? (uint32_t)strtoul(e, nullptr, 10) : 0u, "shrinks the seed pass's compacted lists so that their capacity checks fire (0: off)") \
    X(int64_t,  canon_device_min,   "MAUVE_CANON_DEVICE_MIN",   TEST_KNOB,   e ? atol(e) : 16384, "matches from which the canonical order is made, and a given list chained, on the device") \
    X(int,      ch_big_max,         "MAUVE_CH_BIG_MAX",         TEST_KNOB,   sw_at_least(e ? atoi(e) : 2048, 1), "largest overlap cluster the one-lane chain kernel takes") \
    X(int,      ch_cl_max,          "MAUVE_CH_CL_MAX",          TEST_KNOB,   !e ? 0 : sw_at_least(atoi(e), 1), "largest overlap cluster of the per-lane chain pass; chain_dev.hip caps it at CH_CL_MAX, which unset (0) means") \
    X(bool,     host_chain,         "MAUVE_HOST_CHAIN",         AB,          e != nullptr, "overlap elimination and LCBs on the host, in align and in the progressive nodes") \
    X(bool,     host_tail,          "MAUVE_HOST_TAIL",          AB,          e != nullptr, "chains come back to the host; the interval table is assembled there") \
    X(bool,     host_extend,        "MAUVE_HOST_EXTEND",        AB,          e != nullptr, "LCB extension in match-level rounds on the host") \
    X(bool,     ext_decline,        "MAUVE_EXT_DECLINE",        TEST_KNOB,   e != nullptr, "the device LCB extension hands back its first round with matches as if an LCB had died") \
    X(bool,     given_on_host,      "MAUVE_GIVEN_ON_HOST",      AB,          e != nullptr, "a caller's match list is chained on the host whatever its length") \
    X(bool,     host_gap_chain,     "MAUVE_HOST_GAP_CHAIN",     AB,          e != nullptr, "recursion batches are chained on the host") \
    X(bool,     gap_chain_all_back, "MAUVE_GAP_CHAIN_ALL_BACK", AB,          e != nullptr, "the device chain of a recursion batch copies every record and graph back") \
    X(bool,     shard_single,       "MAUVE_SHARD_SINGLE",       TEST_KNOB,   e != nullptr, "a one-rank RCCL world goes through the sharded path") \
    X(bool,     bb_column_scan,     "MAUVE_BB_COLUMN_SCAN",     AB,          e != nullptr, "the backbone's pair kernel scans the columns itself, without the per-chunk last-column table") \
    X(int,      dp_class,           "MAUVE_DP_CLASS",           AB,          !e ? 0 : !strcmp(e, "bound") ? 1 : !strcmp(e, "wild") ? 2 : 0, "DP size-class estimate: bound (1), wild (2), anything else the default (0)") \
    X(int64_t,  dp_wide_min,        "MAUVE_DP_WIDE_MIN",        TEST_KNOB,   e ? atoll(e) : 1024, "single-wave scan steps from which an interval may get a workgroup") \
    X(int64_t,  dp_big_max,         "MAUVE_DP_BIG_MAX",         TEST_KNOB,   e ? atoll(e) : 256, "most intervals of a batch that get a workgroup") \
    X(int64_t,  dp_cluster,         "MAUVE_DP_CLUSTER",         AB,          e ? atoll(e) : 32, "workgroup entries that get a cluster of workgroups each (0: none)") \
    X(int64_t,  dp_desc_min,        "MAUVE_DP_DESC_MIN",        TEST_KNOB,   e ? atoll(e) : 2048, "intervals from which a descriptor batch takes the device front end") \
    X(int64_t,  dp_tb_budget,       "MAUVE_DP_TB_BUDGET",       TEST_KNOB,   sw_at_least(e ? atoll(e) : 8LL << 30, 65536), "traceback bytes of one DP round; a batch that needs more runs in several rounds") \
    X(bool,     dp_no_wide,         "MAUVE_DP_NO_WIDE",         AB,          e != nullptr, "workgroup entries all go through the stripe pipeline, none through the wide sweep") \
    X(bool,     dp_noscan,          "MAUVE_DP_NOSCAN",          AB,          e != nullptr, "anti-diagonal sweep for the one-wave class too") \
    X(bool,     dp_one_wave,        "MAUVE_DP_ONE_WAVE",        AB,          e != nullptr, "no interval gets a workgroup") \
    X(bool,     dp_no_groups,       "MAUVE_DP_NO_GROUPS",       AB,          e != nullptr, "no interval shares a wave with others") \
    X(bool,     dp_desc_host,       "MAUVE_DP_DESC_HOST",       AB,          e != nullptr, "descriptor batches take the host front end whatever their size")

struct Switches {
#define X(type, field, name, kind, value, doc) type field;
    MAUVE_SWITCHES(X)
#undef X
};

inline const Switches &switches()
{
    static const Switches table = [] {
        Switches s;
#define X(type, field, name, kind, value, doc) { const char *e = getenv(name); s.field = (value); }
        MAUVE_SWITCHES(X)
#undef X
        return s;
    }();
    return table;
}
