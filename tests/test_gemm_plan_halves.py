"""CPU check of the planner's halves rule (tpp-mlir_amd/csrc/gemm_plan.cpp choose_f32_halves, xsmm_hip_set_f32_halves):
tests/gemm_plan_halves/driver.cpp steps f32 calls - C2 and other layers on the 64x64 + K2 tile, the shapes of tests/test_f32_halves_gpu.py,
shapes not in whole 64x64 tiles, every other f32 tile, a forced and a modelled split, the tail split, edge tiles, ragged k, strict mode,
unaligned operands, tile-queue groups - through plan_gemm and plan_gemm_call / plan_gemm_group at 256 and 64 compute units with
GemmPlanEnv::halves = 0, 1 and 2. One line per call and environment; tests/golden/gemm_plan_halves.txt is the reviewed record of the
rule. Whatever the table says, every line must also satisfy the rule's invariants (below)."""
import difflib
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tpp-mlir_amd", "csrc")
GOLDEN = os.path.join(ROOT, "tests", "golden", "gemm_plan_halves.txt")
sys.path.insert(0, os.path.join(ROOT, "tpp-mlir_amd"))
import build  # noqa: E402

LINE = re.compile(r'^(call|group) (\d+)x(\d+)x(\d+) br(\d+) f(-?\d+) cus(\d+) S(-?\d+) T(\d+) E(\d+) K(\d+) strict([01]) al([01]) : v(\d+) (\S+) t(\d+) s(\d+) '
                  r'tail(\d+) e([01]) k([01]) "([^"]*)" "([^"]*)" \| h([01])([01])([01])$')
FIELDS = ("kind", "m", "n", "k", "br", "forced", "cus", "fsplit", "tail_mode", "edge_mode", "edge_k_mode", "strict", "aligned", "variant", "launcher",
          "tile", "split", "tail", "edge", "edge_k", "name", "text", "h0", "h1", "h2")


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    try:
        cc = build.hipcc()
    except RuntimeError as e:
        pytest.fail(str(e))
    d = tmp_path_factory.mktemp("gemm_plan_halves")
    objs = []
    for src, name in ((os.path.join(CSRC, "gemm_plan.cpp"), "gemm_plan.o"), (os.path.join(ROOT, "tests", "gemm_plan_halves", "driver.cpp"), "driver.o")):
        obj = str(d / name)
        subprocess.check_call([cc] + build.FLAGS + ["-x", "hip", "-I" + CSRC, "-c", src, "-o", obj])
        objs.append(obj)
    exe = str(d / "plan_halves")
    subprocess.check_call([cc, "--offload-arch=" + build.ARCH] + objs + ["-o", exe])
    return subprocess.run([exe], capture_output=True, text=True, check=True, timeout=120).stdout


@pytest.fixture(scope="module")
def rows(table):
    """the driver prints a mode's decision as one digit (GemmLaunch::halves) only if everything else - descriptor variant and name,
    launcher, tile, split, text, tail, edge flags - equals the mode-0 decision, and in full behind a "!" otherwise, which LINE does not
    match: the switch never changes which kernel a call is planned on or what it reports"""
    out = []
    for l in table.splitlines():
        m = LINE.match(l)
        assert m, "a decision that differs from mode 0 in more than the halves flag: " + l
        r = dict(zip(FIELDS, m.groups()))
        for k in FIELDS:
            if k not in ("kind", "launcher", "name", "text"):
                r[k] = int(r[k])
        r["line"] = l
        out.append(r)
    return out


def test_planner_reproduces_the_golden_halves_table(table):
    with open(GOLDEN) as f:
        want = f.read()
    if table != want:
        diff = "".join(list(difflib.unified_diff(want.splitlines(True), table.splitlines(True), "golden", "planner"))[:80])
        pytest.fail("the planner's halves choices differ from tests/golden/gemm_plan_halves.txt:\n" + diff)


def eligible(r):
    """the issue's rule, restated: the 64x64 + K2 tile as one plain launch of a single whole-layer call, m and n in whole 64x64 tiles"""
    return (r["kind"] == "call" and r["launcher"] == "f32_lw" and r["tile"] == 1 and r["split"] == 1 and r["tail"] == 0 and not r["edge"]
            and not r["edge_k"] and r["m"] % 64 == 0 and r["n"] % 64 == 0)


def test_every_line_keeps_the_rule(rows):
    for r in rows:
        assert r["h0"] == 0, "mode 0 never: " + r["line"]
        assert r["h2"] == int(eligible(r)), "mode 2 = wherever eligible, nowhere else: " + r["line"]
        tiles = (r["m"] // 64) * (r["n"] // 64)
        assert r["h1"] == int(eligible(r) and tiles >= r["cus"]), "mode 1 = eligible and at least one tile per CU (the measured classes): " + r["line"]
        if r["h2"]:
            assert r["variant"] == 6 and r["text"] == "" and r["name"] == "brgemm_f32_fast_lw<64x64,k2>", r["line"]
    assert sum(r["h2"] for r in rows) >= 30


def test_case_list_covers_what_the_rule_depends_on(rows):
    assert {r["cus"] for r in rows} == {256, 64}
    def some(**kw):
        return [r for r in rows if all(r[k] == v for k, v in kw.items())]
    # C2: tiles <= CUs, the class the rule had to examine; and more tiles than CUs
    c2 = some(kind="call", m=1024, n=1024, k=64, br=16, forced=-1, cus=256, fsplit=-1, tail_mode=0, edge_mode=0, edge_k_mode=0, strict=0, aligned=1)
    assert len(c2) == 1 and c2[0]["h2"] == 1 and c2[0]["h1"] == 1
    assert any(r["h1"] for r in rows if r["cus"] == 64) and any(r["h2"] and not r["h1"] for r in rows), "both sides of the rule's tile count"
    assert any(r["h2"] and (r["m"] // 64) * (r["n"] // 64) > r["cus"] for r in rows)
    # every way out of eligibility appears, on a call that is otherwise planned on the 64x64 + K2 tile where that is possible
    assert any(not r["h2"] and r["n"] % 64 for r in rows) and any(not r["h2"] and r["m"] % 64 for r in rows)
    assert any(not r["h2"] and r["variant"] == 6 and r["split"] > 1 and r["fsplit"] == 2 for r in rows), "a forced split"
    assert any(not r["h2"] and r["variant"] == 6 and r["split"] > 1 and r["fsplit"] == -1 for r in rows), "a modelled split"
    assert any(r["h2"] and r["fsplit"] == 0 for r in rows), "splits forced off"
    assert any(not r["h2"] and r["variant"] == 6 and r["tail"] > 0 for r in rows), "a tail split"
    assert any(r["h2"] and r["tail_mode"] == 1 for r in rows), "the tail split on, a shape without a tail"
    assert any(not r["h2"] and r["edge"] and r["tile"] == 1 for r in rows) and any(r["h2"] and r["edge_mode"] for r in rows)
    assert any(not r["h2"] and r["edge_k"] and r["tile"] == 1 for r in rows) and any(r["h2"] and r["edge_k_mode"] for r in rows)
    assert any(not r["h2"] and r["variant"] == 6 and not r["aligned"] for r in rows), "unaligned operands: the generic kernel"
    assert any(r["h2"] and r["strict"] for r in rows), "strict mode takes the same decision"
    assert {r["tile"] for r in rows if r["launcher"] == "f32_lw" and not r["h2"] and not r["edge"] and not r["edge_k"] and r["split"] == 1
            and r["tail"] == 0} >= {0, 2, 3}, "the other loader-wave tiles"
    groups = some(kind="group")
    assert groups and not any(r["h2"] for r in groups), "a tile-queue group is never taken"
    assert any(r["variant"] == 6 for r in groups)
    # the shapes of tests/test_f32_halves_gpu.py
    for m, n, k, br in ((64, 64, 64, 1), (64, 64, 64, 2), (128, 192, 64, 3), (128, 192, 64, 4), (128, 192, 64, 5), (128, 192, 64, 7), (128, 128, 128, 3),
                        (64, 128, 64, 4), (192, 64, 64, 2), (1088, 1024, 64, 2)):
        for cus in (256, 64):
            got = some(kind="call", m=m, n=n, k=k, br=br, forced=6, cus=cus, fsplit=-1, strict=0)
            assert got and all(r["h2"] for r in got), (m, n, k, br, cus)
