"""The layout of the kernel sources (no GPU): rsx_kernels.hpp holds the four lane-group kernel templates and nothing else, what they
are made of lives in six headers by concern, each usable on its own, and the pieces of a lane-group step that stepping and lookahead
share are stated once, as text fragments both bodies include."""
import os
import re
import subprocess
import tempfile

import pytest

from __graft_entry__ import CSRC, HIPCC_COMMON

HEADERS = ("rsx_lane_map.hpp", "rsx_contact.hpp", "rsx_state_io.hpp", "rsx_hot_args.hpp", "rsx_task.hpp", "rsx_placement.hpp")
FRAGMENTS = ("rsx_step_commands.inc", "rsx_step_wire.inc", "rsx_step_xr.inc")
BODIES = ("rsx_task_step_body.inc", "rsx_plan_body.inc")


def _text(name):
    return open(os.path.join(CSRC, name)).read()


def _code(text):
    """the text without its // comments"""
    return "\n".join(line.split("//")[0] for line in text.splitlines())


def test_kernels_header_holds_the_four_kernels_and_no_device_function():
    code = _code(_text("rsx_kernels.hpp"))
    assert len(re.findall(r"\b__global__\b", code)) == 4
    assert re.findall(r"\bvoid (\w+)\(RSX_HOT_ARGS", code) == ["sim_step_kernel", "sim_step_phys_kernel", "task_step_kernel", "task_step_phys_kernel"]
    assert "__device__" not in code
    for h in HEADERS:
        assert code.count(f'#include "{h}"') == 1, h


def test_each_fragment_is_included_once_by_both_bodies():
    for body in BODIES:
        text = _text(body)
        for frag in FRAGMENTS:
            assert text.count(f'#include "{frag}"') == 1, (body, frag)
    # ... and the lookahead body names its actions as fed ones, ahead of the first fragment
    plan = _text("rsx_plan_body.inc")
    assert plan.count("constexpr bool fed = true;") == 1
    assert plan.index("constexpr bool fed = true;") < plan.index(f'#include "{FRAGMENTS[0]}"')


def test_bodies_restate_nothing_of_the_shared_pieces():
    for body in BODIES:
        text = _text(body)
        for gone in ("vss_wheel(", "ssl_agent_commands<", "wheel_speeds<", "xr[8] ="):
            assert gone not in text, (body, gone)
        # the compile-time observation width is rsx_task.hpp's
        assert not re.search(r"OD_C\s*=\s*NR\s*==\s*0\s*\?", text), body
        assert "TASK == RSX_TASK_SSL_DRIBBLING ? 21" not in text, body
        assert text.count("constexpr int OD_C = obs_dim_c<TASK, NR>();") == 1, body
    task = _text("rsx_task.hpp")
    assert len(re.findall(r"constexpr int obs_dim_c\(\)", task)) == 1
    # each shared piece has one home
    assert sum(_text(f).count("vss_wheel(a0)") for f in FRAGMENTS) == 1
    assert sum(_text(f).count("wheel_speeds<KIND>(") for f in FRAGMENTS) == 1
    assert sum(_text(f).count("xr[8] =") for f in FRAGMENTS) == 1


@pytest.mark.parametrize("header", HEADERS)
def test_header_compiles_as_the_only_include(header):
    includes = [f for f in HIPCC_COMMON if f.startswith("-I")]
    with tempfile.TemporaryDirectory(prefix="rsx_header_probe_") as work:
        unit = os.path.join(work, "only.hip")
        with open(unit, "w") as f:
            f.write(f'#include "{header}"\n')
        p = subprocess.run([os.environ.get("HIPCC", "hipcc"), "--offload-arch=gfx950", "-std=c++17", "-fsyntax-only"] + includes + [unit],
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, cwd=work)
    assert p.returncode == 0, p.stdout[-3000:]
    assert "error:" not in p.stdout, p.stdout[-3000:]
