"""Build-time lint of the kernels whose global loads are inline asm with explicit vmcnt waits (tools/isa_inflight_check.py):
hipcc does not know that such a load's destination registers are in flight until the matching asm wait, and nothing in the
language stops it from copying or reusing them in between -- it did, in three kernels of rounds 4 - 6, each time with clean
source and wrong results on the GPU.  The machine code that ships is the one built here (the GPU box runs the prebuilt
library), so the check runs here, on the ISA of the same sources and flags.  The walk follows the control flow (back edges,
branches around a wait); the snippets below pin that down on hand-written ISA that a walk in layout order passes.  No GPU
needed; the shipped-kernel check is skipped without hipcc."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
LINT = os.path.join(ROOT, "tools", "isa_inflight_check.py")


def _lint(path):
    r = subprocess.run([sys.executable, LINT, str(path)], capture_output=True, text=True)
    return r.returncode, r.stdout


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc here")
@pytest.mark.parametrize("src", ["conv_thin4.hip", "wgrad_tail.hip", "conv_small.hip", "conv_bf3.hip"])
def test_no_instruction_touches_a_register_with_an_asm_load_in_flight(src, tmp_path):
    out = tmp_path / (src + ".s")
    cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-I" + os.path.join(ROOT, "include"),
           "-I" + os.path.join(ROOT, "deep-image-prior_amd", "csrc"), "-S", "--cuda-device-only",
           os.path.join(ROOT, "deep-image-prior_amd", "csrc", src), "-o", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    rc, stdout = _lint(out)
    last = stdout.strip().splitlines()[-1]
    assert rc == 0, stdout[-3000:]
    assert "0 finding(s)" in last and not last.startswith("0 kernel"), last


# Hand-written kernels in the assembler syntax hipcc emits (asm blocks between the ;;#ASMSTART / ;;#ASMEND markers).
# Each buggy one is clean when walked in layout order and wrong on some path of its control flow.

# A rotated loop (latch laid out above its header, as hipcc places it) whose latch copies the destination of a load issued
# in the loop body, before any wait.
LATCH_COPY = """
k_latch_copy:
\ts_mov_b32 s4, 0
\ts_branch .LBB0_2
.LBB0_1:
\tv_mov_b32_e32 v20, v4
.LBB0_2:
\t;;#ASMSTART
\tglobal_load_dwordx4 v[4:7], v[0:1], off
\t;;#ASMEND
\ts_add_i32 s4, s4, 1
\ts_cmp_lt_i32 s4, s5
\ts_cbranch_scc1 .LBB0_1
\t;;#ASMSTART
\ts_waitcnt vmcnt(0)
\t;;#ASMEND
\tv_add_f32_e32 v21, v4, v20
\ts_endpgm
"""

# A branch that skips the asm wait on one path; the join consumes the load.
SKIPPED_WAIT = """
k_skipped_wait:
\t;;#ASMSTART
\tglobal_load_dwordx4 v[4:7], v[0:1], off
\t;;#ASMEND
\ts_cmp_eq_u32 s6, 0
\ts_cbranch_scc1 .LBB1_2
\t;;#ASMSTART
\ts_waitcnt vmcnt(0)
\t;;#ASMEND
.LBB1_2:
\tv_add_f32_e32 v8, v4, v5
\ts_endpgm
"""

# Three rows in flight from the prologue, the header retires the oldest with vmcnt(2); the body reloads that row's registers
# LAST, after an extra load, so the back edge re-enters the header with four loads in flight and the reloaded row among the
# two youngest: the counted wait no longer covers it.
BACK_EDGE_DEEPER = """
k_back_edge_deeper:
\t;;#ASMSTART
\tglobal_load_dwordx4 v[4:7], v[0:1], off
\t;;#ASMEND
\t;;#ASMSTART
\tglobal_load_dwordx4 v[8:11], v[0:1], off
\t;;#ASMEND
\t;;#ASMSTART
\tglobal_load_dwordx4 v[12:15], v[0:1], off
\t;;#ASMEND
.LBB2_1:
\t;;#ASMSTART
\ts_waitcnt vmcnt(2)
\t;;#ASMEND
\tv_add_f32_e32 v20, v4, v5
\t;;#ASMSTART
\ts_waitcnt vmcnt(0)
\t;;#ASMEND
\tv_add_f32_e32 v21, v8, v12
\t;;#ASMSTART
\tglobal_load_dwordx4 v[8:11], v[0:1], off
\t;;#ASMEND
\t;;#ASMSTART
\tglobal_load_dwordx4 v[12:15], v[0:1], off
\t;;#ASMEND
\t;;#ASMSTART
\tglobal_load_dwordx4 v[16:19], v[2:3], off
\t;;#ASMEND
\t;;#ASMSTART
\tglobal_load_dwordx4 v[4:7], v[0:1], off
\t;;#ASMEND
\ts_add_i32 s4, s4, 1
\ts_cmp_lt_i32 s4, s5
\ts_cbranch_scc1 .LBB2_1
\t;;#ASMSTART
\ts_waitcnt vmcnt(0)
\t;;#ASMEND
\ts_endpgm
"""

# Correct: a rotated two-row pipeline, latch above the header, one row in flight under the other's arithmetic; every path
# into the header has the same queue, and the latch touches no register of a load in flight.
ROTATED_OK = """
k_rotated_ok:
\t;;#ASMSTART
\tglobal_load_dwordx4 v[4:7], v[0:1], off
\t;;#ASMEND
\t;;#ASMSTART
\tglobal_load_dwordx4 v[8:11], v[0:1], off
\t;;#ASMEND
\ts_branch .LBB3_2
.LBB3_1:
\tv_mov_b32_e32 v24, v20
\tv_add_u32_e32 v0, 16, v0
.LBB3_2:
\t;;#ASMSTART
\ts_waitcnt vmcnt(1)
\t;;#ASMEND
\tv_add_f32_e32 v20, v4, v5
\t;;#ASMSTART
\tglobal_load_dwordx4 v[4:7], v[0:1], off
\t;;#ASMEND
\t;;#ASMSTART
\ts_waitcnt vmcnt(1)
\t;;#ASMEND
\tv_add_f32_e32 v21, v8, v9
\t;;#ASMSTART
\tglobal_load_dwordx4 v[8:11], v[0:1], off
\t;;#ASMEND
\ts_add_i32 s4, s4, 1
\ts_cmp_lt_i32 s4, s5
\ts_cbranch_scc1 .LBB3_1
\t;;#ASMSTART
\ts_waitcnt vmcnt(0)
\t;;#ASMEND
\ts_endpgm
"""


@pytest.mark.parametrize("snippet,where", [(LATCH_COPY, "v_mov_b32_e32 v20, v4"), (SKIPPED_WAIT, "v_add_f32_e32 v8, v4, v5"),
                                           (BACK_EDGE_DEEPER, "v_add_f32_e32 v20, v4, v5")],
                         ids=["latch_copy", "skipped_wait", "back_edge_deeper"])
def test_control_flow_walk_flags_what_layout_order_misses(snippet, where, tmp_path):
    f = tmp_path / "k.s"
    f.write_text(snippet)
    rc, out = _lint(f)
    assert rc == 1, out
    assert where in out, out
    assert out.strip().splitlines()[-1] != "1 kernel(s) with asm blocks checked, 0 finding(s)", out


def test_back_edge_is_named_in_the_finding(tmp_path):
    f = tmp_path / "k.s"
    f.write_text(LATCH_COPY)
    rc, out = _lint(f)
    assert "back edge .LBB0_2 -> .LBB0_1" in out, out


def test_back_edge_of_a_one_block_loop_is_named(tmp_path):
    f = tmp_path / "k.s"
    f.write_text(BACK_EDGE_DEEPER)
    rc, out = _lint(f)
    assert "back edge .LBB2_1 -> .LBB2_1" in out, out


def test_correct_rotated_loop_stays_clean(tmp_path):
    f = tmp_path / "k.s"
    f.write_text(ROTATED_OK)
    rc, out = _lint(f)
    assert rc == 0, out
    assert out.strip().splitlines()[-1] == "1 kernel(s) with asm blocks checked, 0 finding(s)", out
