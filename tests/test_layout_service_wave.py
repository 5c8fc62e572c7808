"""When a handle's single steps run in the paired form (rsoccer_amd/csrc/rsx_layout.hpp: StepPlan::service_wave), checked without a GPU
the way tests/test_layout_plan.py checks the layouts: a stand-alone program that includes only rsx_layout.hpp and rsx.h, built with the
host compiler, answers a list of queries; the expected answers are written from the rule — VSS-v0 3v3 with eight lanes per env and
literal coefficients, up to RSX_SERVICE_WAVE_MAX_ENVS envs, RSX_SERVICE_WAVE=0|1 overriding the batch size and nothing else."""
import os
import re
import shutil
import subprocess
import tempfile

from test_layout_plan import ROOT, query

PROBE = r"""
#include <cstdio>
#include <cstring>
#include "rsx.h"
#include "rsx_layout.hpp"
int main() {
    rsx::LayoutQuery q{};
    int physics = 0;
    char lay[32], svc[32];
    while (std::scanf("%d %d %d %d %d %d %d %d %d %d %d %31s %31s", &q.task, &q.kind, &q.L, &q.NR, &q.n_blue, &q.num_envs, &q.row_stride,
                      &q.state_dim, &q.obs_dim, &q.n_sub, &physics, lay, svc) == 13) {
        q.physics = physics != 0;
        q.env_layout = std::strcmp(lay, "-") == 0 ? nullptr : lay;
        q.env_service = std::strcmp(svc, "-") == 0 ? nullptr : svc;
        const rsx::StepPlan p = rsx::plan_layout(q);
        std::printf("%d %d\n", (int)p.service_wave, (int)p.step);
    }
    return 0;
}
"""


def threshold():
    text = open(os.path.join(ROOT, "rsoccer_amd", "csrc", "rsx_layout.hpp")).read()
    return int(re.search(r"#define RSX_SERVICE_WAVE_MAX_ENVS (\d+)", text).group(1))


def cases(thr):
    """[(what, query + (override,), expected service_wave)]"""
    out = []
    out.append(("VSS-v0 3v3 at the headline batch, no override", query(1, 4096) + ("-",), 1))
    out.append(("VSS-v0 3v3 at the threshold", query(1, thr) + ("-",), 1))
    out.append(("VSS-v0 3v3, a small batch", query(1, 8) + ("-",), 1))
    out.append(("VSS-v0 3v3 above the threshold", query(1, thr + 1) + ("-",), 0))
    out.append(("VSS-v0 3v3, 65 536 envs", query(1, 65536) + ("-",), 0))
    # the override decides for the eligible handles, at any batch the lane-group kernels step
    out.append(("RSX_SERVICE_WAVE=0 at 4096", query(1, 4096) + ("0",), 0))
    out.append(("RSX_SERVICE_WAVE=1 at 4096", query(1, 4096) + ("1",), 1))
    out.append(("RSX_SERVICE_WAVE=1 at 8192", query(1, 8192) + ("1",), 1))
    out.append(("RSX_SERVICE_WAVE=1, one lane per env", query(1, 1 << 20) + ("1",), 0))
    out.append(("RSX_SERVICE_WAVE=1, RSX_LAYOUT=epl", query(1, 4096, "epl") + ("1",), 0))
    # per-env physics, other widths and team sizes: never
    out.append(("per-env physics", query(1, 4096, physics=True) + ("-",), 0))
    out.append(("per-env physics, RSX_SERVICE_WAVE=1", query(1, 4096, physics=True) + ("1",), 0))
    out.append(("VSS-v0 3v3, 16 lanes per env", query(1, 4096, L=16) + ("1",), 0))
    out.append(("VSS-v0 5v5", query(1, 4096, n_blue=5, n_yellow=5) + ("1",), 0))
    out.append(("VSS-v0 2v4 (run-time robot count)", query(1, 4096, n_blue=2, n_yellow=4) + ("1",), 0))
    for task in (2, 3, 4, 5, 6, 7):   # every other task, asked for or not
        out.append((f"task {task}", query(task, 2048) + ("-",), 0))
        out.append((f"task {task} RSX_SERVICE_WAVE=1", query(task, 2048) + ("1",), 0))
    return out


def test_service_wave_plan_follows_the_rule():
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    thr = threshold()
    assert thr == 4096   # the last batch of the measured crossover table (rsx_layout.hpp) that clears the 2 % bar
    rows = cases(thr)
    work = tempfile.mkdtemp(prefix="rsx_service_probe_")
    try:
        src, exe = os.path.join(work, "probe.cpp"), os.path.join(work, "probe")
        with open(src, "w") as f:
            f.write(PROBE)
        subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                               "-I" + os.path.join(ROOT, "rsoccer_amd", "csrc"), "-o", exe, src])
        feed = "".join(" ".join(str(v) for v in q) + "\n" for _, q, _ in rows)
        p = subprocess.run([exe], input=feed, capture_output=True, text=True, timeout=60)
        assert p.returncode == 0, p.stderr[-2000:]
    finally:
        shutil.rmtree(work, ignore_errors=True)
    got = [line.split() for line in p.stdout.splitlines()]
    assert len(got) == len(rows)
    wrong = [(what, want, g) for (what, _, want), g in zip(rows, got) if int(g[0]) != want]
    assert not wrong, wrong
    # the paired form is a form of the lane-group layout (step == Lanes wherever it is on)
    assert all(int(g[1]) == 0 for g in got if int(g[0]))
