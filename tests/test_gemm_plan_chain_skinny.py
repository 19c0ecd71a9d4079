"""CPU check of the planner's rule for skinny-batch layer chains (tpp-mlir_amd/csrc/gemm_plan.cpp chain_skinny_b_kind / plan_chain_skinny,
xsmm_hip_set_chain_skinny) and of its place in plan_chain: tests/gemm_plan_chain_skinny/driver.cpp, compiled with the library's planner as plain
host C++, prints one line per chain, mode, CU count and strict setting; tests/golden/gemm_plan_chain_skinny.txt is the table. Every 'rule' line
is checked against the rule restated here from the contract in gemm_plan.h; every 'chain' line with m >= 32 must answer as with the new
switch 0, beside each of the seven other chain switches and all of them, and every chain line with m < 32 is the new form's or its gate's."""
import difflib
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tpp-mlir_amd", "csrc")
HIP_INCLUDE = "/opt/rocm/include"
GOLDEN = os.path.join(ROOT, "tests", "golden", "gemm_plan_chain_skinny.txt")
RULE = re.compile(r'^rule m(\d+) n([\d,]+) k([\d,]+) br([\d,]+) img(\d) md(\d+) cus(\d+) st([01]) \| kind(-?\d) bn(\d+) G(\d+) g([01]) "([^"]*)"$')
CHAIN = re.compile(r'^chain m(\d+) n([\d,]+) img(\d) sw-(\w+) sk(\d+) cus(\d+) \| (.*)$')
GATE_BYTES = 2 << 20  # the measured gate of mode 1 (profiles/chain_skinny_ab.txt), restated: see gemm_plan.h plan_chain_skinny


def rule(m, ns, ks, brs, cus, kind, mode, strict):
    """(BN, G, gated) of the launch, None = refused - restated from gemm_plan.h"""
    forced_g = mode // 1000 if mode >= 1000 else 0
    bn = mode % 1000 if mode >= 1000 else mode
    if mode != 1 and (bn not in (16, 32, 64) or (mode >= 1000 and not 1 <= forced_g <= 512)):
        return None
    if not 2 <= len(ns) <= 8 or not 1 <= m <= 31 or kind not in (0, 2, 4) or strict:
        return None
    if any(b < 1 for b in brs) or any(n < 16 or n % 8 for n in ns) or any(k < 8 or k % 8 for k in ks):
        return None
    if mode == 1:
        bn = 32 if kind == 2 else 16
    if (kind == 2 and bn == 16) or min(ns) < bn:
        return None
    if forced_g > cus:
        return None
    G = forced_g or min(max(-(-n // bn) for n in ns), cus)
    gated = mode == 1 and (kind != 0 or max(2 * b * k * n for b, k, n in zip(brs, ks, ns)) > GATE_BYTES)
    return bn, G, gated


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    gxx = shutil.which("g++")
    if not gxx or not os.path.exists(os.path.join(HIP_INCLUDE, "hip", "hip_runtime.h")):
        pytest.skip("needs g++ and the HIP headers")
    d = tmp_path_factory.mktemp("gemm_plan_chain_skinny")
    exe = str(d / "plan_chain_skinny")
    subprocess.check_call([gxx, "-std=c++17", "-O1", "-D__HIP_PLATFORM_AMD__", "-I" + HIP_INCLUDE, "-I" + CSRC, os.path.join(CSRC, "gemm_plan.cpp"),
                           os.path.join(ROOT, "tests", "gemm_plan_chain_skinny", "driver.cpp"), "-o", exe])
    return subprocess.run([exe], capture_output=True, text=True, check=True, timeout=120).stdout


def test_planner_reproduces_the_golden_table(table):
    with open(GOLDEN) as f:
        want = f.read()
    if table != want:
        diff = "".join(list(difflib.unified_diff(want.splitlines(True), table.splitlines(True), "golden", "planner"))[:80])
        pytest.fail("the planner's choices differ from tests/golden/gemm_plan_chain_skinny.txt:\n" + diff)


def test_every_rule_line_keeps_the_rule(table):
    seen = {"taken": 0, "gated": 0, "refused": 0}
    for l in table.splitlines():
        if not l.startswith("rule"):
            continue
        g = RULE.match(l)
        assert g, "unreadable line: " + l
        g = g.groups()
        m, ns, ks, brs = int(g[0]), [int(x) for x in g[1].split(",")], [int(x) for x in g[2].split(",")], [int(x) for x in g[3].split(",")]
        img, mode, cus, strict, kind, bn, G, gated, why = int(g[4]), int(g[5]), int(g[6]), int(g[7]), int(g[8]), int(g[9]), int(g[10]), int(g[11]), g[12]
        assert kind in (img, -1), l
        want = rule(m, ns, ks, brs, cus, kind, mode, strict) if kind >= 0 else None
        if want is None:
            assert (bn, G, gated) == (0, 0, 0) and why, l
            seen["refused"] += 1
        else:
            assert (bn, G, gated) == (want[0], want[1], int(want[2])) and bool(why) == want[2] and G <= cus, (l, want)
            seen["gated" if want[2] else "taken"] += 1
    assert min(seen.values()) > 10, seen


def test_m_below_32_is_the_new_form_s_and_everything_else_answers_as_before(table):
    skinny = others = 0
    for l in table.splitlines():
        if not l.startswith("chain"):
            continue
        g = CHAIN.match(l)
        assert g, "unreadable line: " + l
        m, sk, answer = int(g.group(1)), int(g.group(5)), g.group(7)
        if m >= 32:
            assert answer.endswith("= off") and "DIFFERS" not in answer and not answer.startswith("skinny"), l
            others += 1
        else:
            assert answer.startswith("skinny:") or (sk == 1 and answer.startswith('calls "') and "gate" in l), l
            skinny += answer.startswith("skinny:")
    assert skinny >= 27 and others >= 100, (skinny, others)
