"""The grid planner of the mixed-tile conv launch (csrc/rca_conv_balance.h), compiled for the host alone into a tiny program that
prints one plan per line.  No GPU: the header is plain C++."""
import itertools
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "realtime_codec_agent_amd", "csrc", "rca_conv_balance.h")

MAIN = r"""
#include <stdio.h>
#include <stdlib.h>
#include "rca_conv_balance.h"
// stdin: "p total n_co simds occ wm wn" -> plan; "f total wm wn text" -> forced plan (RCA_CONV_BALANCE_PLAN syntax)
int main() {
    char kind[4], text[64];
    long total;
    int n_co, simds, occ, wm, wn;
    while (scanf("%3s", kind) == 1) {
        if (kind[0] == 'p') {
            if (scanf("%ld %d %d %d %d %d", &total, &n_co, &simds, &occ, &wm, &wn) != 6) return 2;
            const ConvBalancePlan p = conv_balance_plan(total, n_co, simds, occ, wm, wn);
            printf("%ld %d %d %ld %ld\n", p.bulk_col_tiles, p.fine_wm, p.fine_wn, p.finish, p.finish_single);
        } else {
            if (scanf("%ld %d %d %63s", &total, &wm, &wn, text) != 4) return 2;
            ConvBalancePlan p{-1, -1, -1, 0, 0};
            const bool ok = conv_balance_parse(text, total, wm, wn, &p);
            printf("%d %ld %d %d\n", ok ? 1 : 0, p.bulk_col_tiles, p.fine_wm, p.fine_wn);
        }
    }
    return 0;
}
"""


@pytest.fixture(scope="module")
def planner(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "a host C++ compiler is needed to build the planner"
    d = tmp_path_factory.mktemp("conv_balance")
    src, exe = d / "plan_main.cpp", d / "plan_main"
    src.write_text(MAIN)
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.dirname(HEADER), str(src), "-o", str(exe)])

    def run(lines):
        out = subprocess.run([str(exe)], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout
        rows = [tuple(int(v) for v in ln.split()) for ln in out.splitlines()]
        assert len(rows) == len(lines)
        return rows
    return run


SHAPES = [(2, 2), (1, 2)]   # bulk wave tiles in units of 32: 64 x 64 and 32 x 64


def _grid():
    totals = [1, 7, 8, 9, 64, 127, 128, 129, 258, 400, 513, 1032, 2064, 3200, 4097, 10320, 16000]
    return [(t, n_co, simds, occ, wm, wn)
            for t, n_co, simds, occ, (wm, wn) in itertools.product(totals, [1, 2, 4, 8, 16], [1024, 416], [2, 3], SHAPES)]


def test_plans_cover_every_column_once_and_never_model_slower(planner):
    cases = _grid()
    plans = planner(["p %d %d %d %d %d %d" % c for c in cases])
    mixed = 0
    for (total, n_co, simds, occ, wm, wn), (bulk, fwm, fwn, finish, single) in zip(cases, plans):
        key = (total, n_co, simds, occ, wm, wn)
        waves = total * n_co
        assert single == -(-waves // simds) * wm * wn, key
        assert finish <= single, key
        if waves < simds * occ:                      # under one round: today's grid
            assert (bulk, fwm, fwn) == (total, 0, 0) and finish == single, key
            continue
        if fwn == 0:                                 # the single-shape grid: every column tile is a bulk tile
            assert bulk == total and fwm == 0 and finish == single, key
            continue
        mixed += 1
        assert bulk % 8 == 0 and 0 < bulk < total, key
        assert (fwm, fwn) in ((1, 2), (1, 1)) and fwm * fwn < wm * wn, key
        # the bulk is whole rounds of resident waves (rounded down to 8 column tiles), at most one round short of the launch's
        rounds = waves // (simds * occ)
        assert bulk in {(r * simds * occ // n_co) // 8 * 8 for r in (rounds, rounds - 1) if r >= 1}, key
        # coverage: bulk tiles hold the columns [0, bulk * wn * 32), fine tiles the rest, each exactly once
        fine_tiles = (total - bulk) * wn // fwn
        assert bulk * wn * 32 + fine_tiles * fwn * 32 == total * wn * 32, key
        # the model: MFMAs on the most loaded SIMD, waves dealt evenly
        fine_waves = fine_tiles * n_co * (wm // fwm)
        assert finish == -(-(bulk * n_co) // simds) * wm * wn + -(-fine_waves // simds) * fwm * fwn, key
        assert finish < single, key
    assert mixed > 50    # the grid reaches the mixed plans


def test_headline_plans_on_a_1024_simd_device(planner):
    """The three strided layers of the 256-window step: k16s8 (400 column tiles of 32 x 64 over 16 channel tiles, 3 waves per SIMD),
    k10s5 (3 200 of 64 x 64 over 4, 2 per SIMD) and k8s4 (16 000 of 64 x 64 over 2, 2 per SIMD)."""
    k16, k10, k8 = planner(["p 400 16 1024 3 1 2", "p 3200 4 1024 2 2 2", "p 16000 2 1024 2 2 2"])
    assert k16[:3] == (384, 1, 1)                    # 6 144 bulk waves (2 rounds), 16 tiles of 64 columns as 512 waves of 32 x 32
    assert (400 - 384) * 2 * 16 == 512
    assert k10[0] == 3072 and k10[1:3] in ((1, 2), (1, 1))   # 1 024 waves of 32 x 64 (one per SIMD) or 2 048 of 32 x 32: the same model
    assert k8[:3] == (15360, 1, 1)                   # 640 tiles of 64 columns as 5 120 waves of 32 x 32
    assert (16000 - 15360) * 2 * 2 * 2 == 5120
    for p in (k16, k10, k8):
        assert p[3] < p[4]


def test_forced_plan_text(planner):
    rows = planner([
        "f 1032 1 2 512:32x32", "f 1032 1 2 0:32x32", "f 1032 1 2 1032:32x32", "f 1032 1 2 1024:32x32", "f 1032 1 2 9999:32x32",
        "f 1032 1 2 515:32x32", "f 1032 1 2 512:32x64", "f 1032 2 2 512:32x64", "f 1032 2 2 512:32x32", "f 1032 2 2 512:64x64",
        "f 1032 2 2 x:32x32", "f 1032 2 2 512", "f 1032 2 2 512:32x32x",
    ])
    assert rows[0] == (1, 512, 1, 1)
    assert rows[1] == (1, 0, 1, 1)                   # all fine tiles
    assert rows[2] == (1, 1032, 0, 0)                # no remainder: the single-shape grid
    assert rows[3] == (1, 1024, 1, 1)
    assert rows[4] == (1, 1032, 0, 0)                # clamped to the launch
    assert rows[5] == (1, 512, 1, 1)                 # rounded down to 8 column tiles
    assert rows[6][0] == 0                           # 32 x 64 is not finer than a 32 x 64 bulk
    assert rows[7] == (1, 512, 1, 2)
    assert rows[8] == (1, 512, 1, 1)
    assert all(r[0] == 0 for r in rows[9:])
