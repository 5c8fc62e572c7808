"""Which kernel layout steps a handle (rsoccer_amd/csrc/rsx_layout.hpp: plan_layout), checked without a GPU: a stand-alone program that
includes only rsx_layout.hpp and rsx.h is built with the host compiler, once plain and once with the address and undefined-behaviour
sanitizers, fed a list of queries, and its answers are compared with the table below — written from the thresholds as they stand,
not from the function.  tests/test_gpu_envs.py::test_layout_names_at_thresholds holds rsx_task_layout on real handles to TASKS."""
import os
import shutil
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROBE = r"""
#include <cstdio>
#include <cstring>
#include "rsx.h"
#include "rsx_layout.hpp"
int main() {
    static const char* const names[] = {"Lanes", "LanesBig", "Quad", "Epl"};
    rsx::LayoutQuery q{};
    int physics = 0;
    char lay[32];
    while (std::scanf("%d %d %d %d %d %d %d %d %d %d %d %31s", &q.task, &q.kind, &q.L, &q.NR, &q.n_blue, &q.num_envs, &q.row_stride,
                      &q.state_dim, &q.obs_dim, &q.n_sub, &physics, lay) == 12) {
        q.physics = physics != 0;
        q.env_layout = std::strcmp(lay, "-") == 0 ? nullptr : lay;
        const rsx::StepPlan p = rsx::plan_layout(q);
        std::printf("%s %s %d\n", names[(int)p.step], names[(int)p.rollout], (int)p.rollout_as_steps);
    }
    return 0;
}
"""

# the seven tasks: (name, kind, field_type, n_blue, n_yellow, task id, smallest batch of the automatic large-batch layout,
# rsx_task_layout's name from that batch on, and below it).  Thresholds: the measured crossovers of rsx_layout.hpp
TASKS = (
    ("VSS-v0", 0, 0, 3, 3, 1, 98304, "one-lane-per-env", "8-lanes-per-env"),
    ("static defenders 1v6", 1, 2, 1, 6, 2, 65536, "one-lane-per-env", "8-lanes-per-env"),
    ("dribbling", 1, 2, 1, 4, 3, 49152, "one-lane-per-env", "8-lanes-per-env"),
    ("contested possession", 1, 2, 1, 1, 4, 32768, "one-lane-per-env", "8-lanes-per-env"),
    ("pass endurance", 1, 2, 2, 0, 5, 32768, "one-lane-per-env", "8-lanes-per-env"),
    ("scrimmage 11v11", 1, 1, 11, 11, 6, 32768, "four-lanes-per-env", "32-lanes-per-env-large-batch"),
    ("crowded scrimmage 11v11", 1, 1, 11, 11, 7, 65536, "four-lanes-per-env", "32-lanes-per-env-large-batch"),
)
BY_ID = {t[5]: t for t in TASKS}
BIG_MIN = 8192                                  # large-batch build of the 32-lane scrimmage kernel
ROLLOUT_AS_STEPS_MIN = {6: 49152, 7: 196608}    # a four-lane handle's rollouts become single steps


def query(task, num_envs, layout=None, *, physics=False, n_blue=None, n_yellow=None, L=None, n_sub=5, row_stride=None):
    """the LayoutQuery rsx_task_attach builds for such a handle (25 ms steps: five sub-steps; no row pad below 786 432 envs)"""
    _, kind, _, nb, ny, _, _, _, _ = BY_ID[task]
    nb = nb if n_blue is None else n_blue
    ny = ny if n_yellow is None else n_yellow
    n = nb + ny
    lanes = L or (8 if n + 1 <= 8 else 16 if n + 1 <= 16 else 32)
    nr = {(0, 6, 8): 6, (0, 6, 16): 6, (1, 7, 8): 7, (1, 7, 16): 7, (1, 22, 32): 22}.get((kind, n, lanes), 0)
    if kind == 0 and n == 6 and nb != 3:
        nr = 0
    state_dim = 5 + (6 if kind == 0 else 11) * n
    obs_dim = {1: 4 + 7 * nb + 5 * ny, 2: 4 + 8 * nb + 2 * ny, 3: 5 + 8 * nb + 2 * ny, 4: 4 + 8 * nb + 2 * ny, 5: 4 + 6 * nb,
               6: 2 + 2 * n, 7: 2 + 2 * n}[task]
    return (task, kind, lanes, nr, nb, num_envs, row_stride or num_envs, state_dim, obs_dim, n_sub, int(physics), layout or "-")


def cases():
    """[(what, query, (step, rollout, rollout_as_steps))]"""
    out = []
    for name, _, _, _, _, task, thr, _, _ in TASKS[:5]:   # the five registered tasks: one lane per env from the crossover on
        for n in (thr - 1, thr):
            auto = "Epl" if n >= thr else "Lanes"
            out.append((f"{name} {n}", query(task, n), (auto, auto, 0)))
            out.append((f"{name} {n} RSX_LAYOUT=epl", query(task, n, "epl"), ("Epl", "Epl", 0)))
            out.append((f"{name} {n} RSX_LAYOUT=lanes", query(task, n, "lanes"), ("Lanes", "Lanes", 0)))
    for name, _, _, _, _, task, thr, _, _ in TASKS[5:]:   # both scrimmage line-ups
        for n in (BIG_MIN - 1, BIG_MIN, thr - 1, thr):
            rollout = "LanesBig" if n >= BIG_MIN else "Lanes"
            as_steps = int(n >= ROLLOUT_AS_STEPS_MIN[task])
            out.append((f"{name} {n}", query(task, n), ("Quad" if n >= thr else rollout, rollout, as_steps if n >= thr else 0)))
            out.append((f"{name} {n} RSX_LAYOUT=quad", query(task, n, "quad"), ("Quad", rollout, as_steps)))
            # `lanes` switches the four-lane kernel off and leaves the large-batch build on
            out.append((f"{name} {n} RSX_LAYOUT=lanes", query(task, n, "lanes"), (rollout, rollout, 0)))
        for n in (ROLLOUT_AS_STEPS_MIN[task] - 1, ROLLOUT_AS_STEPS_MIN[task]):
            out.append((f"{name} {n} rollout", query(task, n), ("Quad", "LanesBig", int(n >= ROLLOUT_AS_STEPS_MIN[task]))))
    # 11v11 kernels are built for 11 blue robots and a real time step: no four-lane layout otherwise, asked for or not
    out.append(("scrimmage 10v12", query(6, 65536, n_blue=10, n_yellow=12), ("LanesBig", "LanesBig", 0)))
    out.append(("scrimmage 10v12 RSX_LAYOUT=quad", query(6, 65536, "quad", n_blue=10, n_yellow=12), ("LanesBig", "LanesBig", 0)))
    out.append(("scrimmage, time step 0", query(6, 65536, n_sub=0), ("LanesBig", "LanesBig", 0)))
    out.append(("scrimmage, time step 0, RSX_LAYOUT=quad", query(7, 262144, "quad", n_sub=0), ("LanesBig", "LanesBig", 0)))
    # VSS-v0 with 16 lanes per env (RSX_LANES_PER_ENV=16): never one lane per env
    out.append(("VSS-v0 L=16", query(1, 200000, L=16), ("Lanes", "Lanes", 0)))
    out.append(("VSS-v0 L=16 RSX_LAYOUT=epl", query(1, 200000, "epl", L=16), ("Lanes", "Lanes", 0)))
    # per-env physics: the lane-group kernels whatever the batch and the environment say
    for task, n, lay in ((1, 1 << 20, None), (1, 64, "epl"), (2, 1 << 20, None), (5, 1 << 20, "epl"), (6, 262144, None), (7, 262144, "quad")):
        out.append((f"physics, task {task} {n} {lay}", query(task, n, lay, physics=True), ("Lanes", "Lanes", 0)))
    # 1v6: 84 state rows (29 aux rows); arrays of 2 GB and more (32-bit byte offsets) stay with the lane-group kernels
    below, reach = 6391320, 6391321
    assert 84 * below * 4 < 2 ** 31 <= 84 * reach * 4
    out.append(("1v6 just below 2 GB", query(2, below - 65600, row_stride=below), ("Epl", "Epl", 0)))
    out.append(("1v6 arrays reach 2 GB", query(2, reach - 65600, row_stride=reach), ("Lanes", "Lanes", 0)))
    out.append(("1v6 arrays reach 2 GB, RSX_LAYOUT=epl", query(2, reach - 65600, "epl", row_stride=reach), ("Lanes", "Lanes", 0)))
    return out


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan-ubsan"])
def test_plan_layout_matches_the_threshold_table(sanitize):
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    rows = cases()
    work = tempfile.mkdtemp(prefix="rsx_layout_probe_")
    try:
        src, exe = os.path.join(work, "probe.cpp"), os.path.join(work, "probe")
        with open(src, "w") as f:
            f.write(PROBE)
        flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if sanitize else []
        subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-Werror"] + flags + ["-I" + os.path.join(ROOT, "include"),
                               "-I" + os.path.join(ROOT, "rsoccer_amd", "csrc"), "-o", exe, src])
        feed = "".join(" ".join(str(v) for v in q) + "\n" for _, q, _ in rows)
        p = subprocess.run([exe], input=feed, capture_output=True, text=True, timeout=60)   # the binary itself: no preloaded runtime
        assert p.returncode == 0, p.stderr[-2000:]
    finally:
        shutil.rmtree(work, ignore_errors=True)
    got = [tuple(line.split()) for line in p.stdout.splitlines()]
    assert len(got) == len(rows)
    wrong = [(what, want, g) for (what, _, want), g in zip(rows, got) if g != (want[0], want[1], str(want[2]))]
    assert not wrong, wrong
