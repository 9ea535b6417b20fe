"""The include graph of csrc/ and its headers on their own (CPU only; the preprocessor and -fsyntax-only, nothing
is compiled to code):

* which unit sees which header, from `hipcc -MM` of every kernel unit (*.hip) and host unit (gol_*.cpp): a unit
  sees what it uses.  The descriptor headers and the step kernels' machinery reach the units that hold those
  kernels and no other, the batch's host units see nothing of the board engine, and no header gathers every
  launcher header again;
* every header of csrc/ compiles when it is the only thing a unit includes: the eight shared with the HIP-free
  stand-alone programs as plain C++ with g++ and no ROCm include path, the others as HIP (those with device code
  for the device, the rest for the host).
"""
import glob
import os
import re
import shutil
import subprocess
from concurrent.futures import ThreadPoolExecutor

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gol-distributed-final_amd", "csrc")
INC = os.path.join(ROOT, "include")
HIPCC = "/opt/rocm/bin/hipcc"
FLAGS = ["-std=c++17", "-I" + INC, "-I" + CSRC]
pytestmark = pytest.mark.skipif(shutil.which(HIPCC) is None, reason="hipcc not present")

# shared with plain C++ programs (tests/san): no hip_runtime.h, directly or through another header
HIP_FREE = ("gol_batch.h", "gol_island.h", "gol_map.h", "gol_rule.h", "gol_edit.h", "gol_copy.h", "gol_strips.h",
            "gol_step_launch.h")
STEP_UNITS = {"gol_kernels.hip", "gol_band_pipe.hip", "gol_bytes_pipe.hip"}
PIPE_UNITS = {"gol_band_pipe.hip", "gol_bytes_pipe.hip"}
REGION_UNITS = {"gol_view.hip", "gol_edit.hip", "gol_copy.hip"}
BATCH_UTIL_UNITS = {"gol_batch.hip", "gol_batch_map.hip", "gol_batch_pass.hip", "gol_island.hip", "gol_util.hip"}
BATCH_HOST_UNITS = {"gol_batch_engine.cpp", "gol_batch_census.cpp"}


def headers():
    return sorted(os.path.basename(p) for p in glob.glob(os.path.join(CSRC, "*.h")))


def pool(fn, items):
    with ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as ex:
        return dict(zip(items, ex.map(fn, items)))


@pytest.fixture(scope="module")
def graph():
    """unit -> the headers of csrc/ it depends on (by file name)."""
    units = sorted(os.path.basename(p) for pat in ("*.hip", "gol_*.cpp") for p in glob.glob(os.path.join(CSRC, pat)))
    own = set(headers())

    def deps(unit):
        arch = ["--offload-arch=gfx950"] if unit.endswith(".hip") else []
        r = subprocess.run([HIPCC] + arch + FLAGS + ["-MM", os.path.join(CSRC, unit)], capture_output=True, text=True)
        assert r.returncode == 0, unit + ": " + r.stderr[-2000:]
        return {os.path.basename(w) for w in r.stdout.replace("\\\n", " ").split()} & own
    return pool(deps, units)


def test_every_unit_is_in_the_graph(graph):
    kernel = {u for u in graph if u.endswith(".hip")}
    assert STEP_UNITS | REGION_UNITS | BATCH_UTIL_UNITS == kernel, sorted(kernel)
    assert BATCH_HOST_UNITS <= set(graph) and len(graph) - len(kernel) >= 21
    assert all(graph[u] for u in kernel)  # (a parse of the dependency output that found nothing would pass every ban)


def test_a_unit_sees_what_it_uses(graph):
    kernel = {u for u in graph if u.endswith(".hip")}
    bans = []  # (the units, the headers none of them may see)
    bans.append((kernel - REGION_UNITS, {"gol_edit.h"}))
    bans.append((kernel - STEP_UNITS, {"gol_step_launch.h", "gol_strips.h", "gol_step_device.h"}))
    bans.append((kernel - PIPE_UNITS, {"gol_pipe.h"}))
    bans.append((BATCH_UTIL_UNITS, {"gol_edit.h", "gol_copy.h", "gol_step_launch.h", "gol_strips.h", "gol_pipe.h"}))
    bans.append((BATCH_HOST_UNITS, {"gol_engine_int.h", "gol_comm.h", "gol_edit.h", "gol_strips.h", "gol_step_launch.h"}))
    seen = sorted({"%s sees %s" % (u, h) for units, banned in bans for u in units for h in graph[u] & banned})
    assert not seen, "\n".join(seen)
    # and the headers are reached where they are used (the names above are those of files that exist)
    for units, h in ((REGION_UNITS, "gol_edit.h"), (STEP_UNITS, "gol_step_device.h"), (STEP_UNITS, "gol_strips.h"),
                     ({"gol_kernels.hip"}, "gol_step_launch.h"), (PIPE_UNITS, "gol_pipe.h")):
        assert all(h in graph[u] for u in units), h


LAUNCHER_HEADERS = {"gol_step_kernels.h", "gol_util_kernels.h", "gol_region_kernels.h", "gol_batch_kernels.h"}


def umbrellas(text):
    """The headers of `text` (name -> source) that include every launcher header, directly or through others."""
    direct = {h: set(re.findall(r'^\s*#\s*include\s+"([^"]+)"', t, re.M)) & set(text) for h, t in text.items()}

    def closure(h, seen):
        for d in direct[h] - seen:
            seen.add(d)
            closure(d, seen)
        return seen
    return sorted(h for h in text if LAUNCHER_HEADERS <= closure(h, {h}))


def test_no_header_gathers_the_launcher_headers():
    """The launcher headers are the host headers that declare a golk_ launcher (a function that returns hipError_t),
    one per family of units: the step, the util and IPC, the region and the batch kernels.  gol_launch.h holds the
    launch state and gol_step_device.h is device code; neither is one.  No header of csrc/ includes all four."""
    text = {h: open(os.path.join(CSRC, h)).read() for h in headers()}
    found = {h for h, t in text.items()
             if re.search(r"^hipError_t golk_\w+\(", t, re.M) and "__device__" not in t and h != "gol_launch.h"}
    assert found == LAUNCHER_HEADERS, sorted(found ^ LAUNCHER_HEADERS)  # (a new family's header is named above)
    assert not umbrellas(text), "%s include(s) every launcher header" % ", ".join(umbrellas(text))
    # the check finds what it looks for: the header that was split, and one that reaches it through another
    every = "".join('#include "%s"\n' % h for h in sorted(LAUNCHER_HEADERS))
    assert umbrellas(dict(text, **{"gol_all.h": every})) == ["gol_all.h"]
    assert umbrellas(dict(text, **{"gol_all.h": every, "gol_more.h": '#include "gol_all.h"\n'})) == ["gol_all.h", "gol_more.h"]
    three = "".join('#include "%s"\n' % h for h in sorted(LAUNCHER_HEADERS)[:3])
    assert not umbrellas(dict(text, **{"gol_three.h": three}))


def syntax_only(tmp_path, header, cmd):
    src = tmp_path / (header[:-2] + "_only.cpp")
    src.write_text('#include "%s"\n' % header)
    r = subprocess.run(cmd + ["-fsyntax-only", str(src)], capture_output=True, text=True)
    return "" if r.returncode == 0 else "%s: %s" % (header, r.stderr[-1500:])


def test_hip_free_headers_compile_alone_as_plain_cpp(tmp_path):
    assert set(HIP_FREE) <= set(headers())
    # g++, or ROCm's clang++ under its own name: neither driver adds a ROCm include path, as hipcc does
    cxx = shutil.which("g++") or shutil.which("/opt/rocm/lib/llvm/bin/clang++")
    assert cxx, "no plain C++ compiler"
    bad = pool(lambda h: syntax_only(tmp_path, h, [cxx, "-Wall"] + FLAGS), list(HIP_FREE))
    assert not any(bad.values()), "\n".join(v for v in bad.values() if v)


def test_hip_headers_compile_alone(tmp_path):
    rest = [h for h in headers() if h not in HIP_FREE]
    assert len(rest) >= 10

    def check(h):
        device = "__device__" in open(os.path.join(CSRC, h)).read()
        side = ["--offload-arch=gfx950", "--cuda-device-only"] if device else ["--cuda-host-only"]
        return syntax_only(tmp_path, h, [HIPCC, "-x", "hip", "-Wall"] + side + FLAGS)
    bad = pool(check, rest)
    assert not any(bad.values()), "\n".join(v for v in bad.values() if v)
