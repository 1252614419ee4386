"""CPU: the captured-graph cache's policy (csrc/graph_cache.h), driven through tests/native/graph_cache_check.cpp, and the public
boundary of zv_set_graph_cache / zv_graph_cache_stats without a GPU.

The check program replays 24 000 seeded operations — lookup, capture, epoch bump, lane drop, capacity change, retire / sweep with
events that complete at chosen times, full drop — through the header and through a model of the rules written out beside it, and
compares after every step: the slot set and the victim, lookups = hits + captures, captures = entries + evictions + stale_evictions +
lane_drops + full_drops, entries <= capacity, that a stale slot goes before a live one, that a hit leaves the slot set alone, that a
colliding hash with another key is a miss, that the retire list stays within the capacity, waits for its oldest entry alone and that
no exec is destroyed before its event completes, or twice, or never.  Once more through a build with
-fsanitize=address,undefined, as a stand-alone program."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "zerovox.cpp_amd", "csrc")
CHECK = os.path.join(ROOT, "tests", "native", "graph_cache_check.cpp")


def _build(tmp, name, extra, inc=()):
    out = str(tmp / name)
    r = subprocess.run(["g++", "-O2", "-g", "-std=c++17", "-Wall", "-Werror"] + ["-I" + i for i in inc] + ["-I" + CSRC] + extra + [CHECK, "-o", out],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    return out


@pytest.fixture(scope="module")
def exes(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("graph_cache")
    return _build(tmp, "graph_cache_check", []), _build(tmp, "graph_cache_check_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])


def test_policy_follows_the_written_out_model(exes):
    r = subprocess.run([exes[0], "cases"], capture_output=True, text=True, timeout=120)
    # 24 000 operations, a dozen or more single checks behind each
    assert r.returncode == 0 and r.stdout.split()[0] == "ok" and int(r.stdout.split()[1]) >= 200000, (r.stdout[-1000:], r.stderr[-500:])


def test_header_under_address_and_undefined_sanitizers(exes):
    r = subprocess.run([exes[1], "cases"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.split()[0] == "ok", (r.stdout[-1000:], r.stderr[-3000:])
    assert "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr[-3000:]


@pytest.mark.parametrize("name,old,new", [
    # a hit decided by the hash alone: a collision replays another key's graph
    ("collision", "if (slots_[i].hash == hash && same(items_[i])) return (int)i;", "if (slots_[i].hash == hash) return (int)i;"),
    # no preference for slots of an older epoch
    ("stale", "if (best < 0 || (stale && !best_stale) || (stale == best_stale && ", "if (best < 0 || ("),
    # the most recently used goes
    ("lru", "slots_[i].tick < slots_[(size_t)best].tick", "slots_[i].tick > slots_[(size_t)best].tick"),
    # a hit that does not count as a use
    ("touch", "        slots_[(size_t)i].tick = ++tick_;\n", ""),
    # a lane drop that takes every lane's slots
    ("lane", "if (slots_[i].lane == lane)", "if (slots_[i].lane >= 0)"),
    # a retire list that grows past its bound
    ("bound", "while (list_.size() >= bound)", "while (list_.size() > bound)"),
    # a full retire list that destroys its oldest entry without waiting for it
    ("wait", "            wait(list_.front());\n", ""),
    # a shrink that evicts nothing
    ("shrink", "        while (slots_.size() > capacity_) evict(epoch, out);\n", ""),
])
def test_the_check_program_sees_a_wrong_header(tmp_path, name, old, new):
    """the same program over a header with one mistake in the policy fails: the check is not vacuous"""
    h = open(os.path.join(CSRC, "graph_cache.h")).read()
    assert h.count(old) == 1, name
    (tmp_path / "graph_cache.h").write_text(h.replace(old, new))
    r = subprocess.run(["g++", "-O1", "-std=c++17", "-w", "-I" + str(tmp_path), "-I" + CSRC, CHECK, "-o", str(tmp_path / "bad")],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(tmp_path / "bad"), "cases"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "FAILED" in r.stdout and "ok" not in r.stdout.split(), r.stdout[-500:]


def test_graph_stats_struct_has_the_headers_fields_at_the_headers_offsets():
    """capi.GraphStats against the typedef in include/zerovox_amd.h: the same names in the same order, uint32 / uint64 as declared,
    at the offsets a C compiler gives them (four uint32, then uint64s: no padding)"""
    from zerovox_cpp_amd import capi
    header = open(os.path.join(ROOT, "include", "zerovox_amd.h")).read()
    body = re.search(r"typedef struct\s*\{([^}]*)\}\s*zv_graph_stats;", header)
    assert body, "zv_graph_stats not found in the header"
    decl = re.sub(r"/\*.*?\*/", "", body.group(1), flags=re.S)
    want, off = [], 0
    for ctype, names in re.findall(r"(uint32_t|uint64_t)\s+([^;]+);", decl):
        size = 4 if ctype == "uint32_t" else 8
        for n in names.split(","):
            off = (off + size - 1) // size * size
            want.append((n.strip(), size, off))
            off += size
    assert [w[0] for w in want] == ["capacity", "entries", "retired", "reserved", "lookups", "hits", "captures", "evictions",
                                    "stale_evictions", "lane_drops", "full_drops"]
    got = [(n, C.sizeof(t), getattr(capi.GraphStats, n).offset) for n, t in capi.GraphStats._fields_]
    assert got == want
    assert C.sizeof(capi.GraphStats) == off == 72


def test_both_calls_refuse_a_null_model_with_a_message():
    from zerovox_cpp_amd import capi
    lib = capi.load_library()
    st = capi.GraphStats()
    for call in (lambda: lib.zv_set_graph_cache(None, 16), lambda: lib.zv_graph_cache_stats(None, C.byref(st))):
        assert call() == 5                                   # ZV_ERR_ARG
        assert b"null" in lib.zv_last_error()
    assert {"zv_set_graph_cache", "zv_graph_cache_stats"} <= set(capi.SYMBOLS)
