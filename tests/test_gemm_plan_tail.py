"""CPU check of the planner's tail-split rule (tpp-mlir_amd/csrc/gemm_plan.cpp choose_f32_tail_split, xsmm_hip_set_tail_split):
tests/gemm_plan_tail/driver.cpp steps whole-layer f32 calls - the reference's 34 f32 benchmark layers, 2.5 / 1.5 / 1.25-round outputs,
one round, a skinny output, 272 tiles of each K-split tile, batch counts around the rule's thresholds - through plan_gemm and
plan_gemm_call at 256, 304 and 64 compute units, tail-split modes 0, 1, 2, 4 and 16, forced split counts -1, 0 and 2, strict mode on
and off, the three K-split tiles forced and as planned. One line per call and environment, with the decision under every mode; tests/golden/gemm_plan_tail.txt is the reviewed record
of the rule. Whatever the table says, every line must also satisfy the rule's invariants (below)."""
import difflib
import json
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tpp-mlir_amd", "csrc")
GOLDEN = os.path.join(ROOT, "tests", "golden", "gemm_plan_tail.txt")
sys.path.insert(0, os.path.join(ROOT, "tpp-mlir_amd"))
import build  # noqa: E402

LINE = re.compile(r'^(\d+)x(\d+)x(\d+) e(\S+) f(-?\d+) cus(\d+) S(-?\d+) strict([01]) : v(\d+) tiles(\d+) chunks(\d+) (\S+) t(\d+) s(\d+) "([^"]*)" \|'
                  r'((?: \d+:(?:-|\d+x\d+))+)(?: \| "([^"]*)")?$')
FIELDS = ("m", "n", "k", "ep", "forced", "cus", "fsplit", "strict", "variant", "tiles", "chunks", "launcher", "tile", "split", "text")


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    try:
        cc = build.hipcc()
    except RuntimeError as e:
        pytest.fail(str(e))
    d = tmp_path_factory.mktemp("gemm_plan_tail")
    objs = []
    for src, name in ((os.path.join(CSRC, "gemm_plan.cpp"), "gemm_plan.o"), (os.path.join(ROOT, "tests", "gemm_plan_tail", "driver.cpp"), "driver.o")):
        obj = str(d / name)
        subprocess.check_call([cc] + build.FLAGS + ["-x", "hip", "-I" + CSRC, "-c", src, "-o", obj])
        objs.append(obj)
    exe = str(d / "plan_tail")
    subprocess.check_call([cc, "--offload-arch=" + build.ARCH] + objs + ["-o", exe])
    return subprocess.run([exe], capture_output=True, text=True, check=True, timeout=120).stdout


@pytest.fixture(scope="module")
def rows(table):
    """one row per line and mode. The driver prints a mode's decision as "-" only if launcher, tile, split, text and every other field
    equal the mode-0 decision of the line and there is no tail, as "<tail tiles>x<workgroups>" only for the same launcher and tile with
    split 1, and anything else in full behind a "!" - which LINE does not match"""
    out = []
    for l in table.splitlines():
        m = LINE.match(l)
        assert m, "a decision that is neither today's nor a tail split of today's kernel: " + l
        base = dict(zip(FIELDS, m.groups()[:15]))
        for k in FIELDS:
            if k not in ("ep", "launcher", "text"):
                base[k] = int(base[k])
        modes = [x.split(":") for x in m.group(16).split()]
        assert [int(a) for a, _ in modes] == [0, 1, 2, 4, 16], l
        for mode, dec in modes:
            r = dict(base, mode=int(mode), line=l, br=base["k"] // 64, tail_tiles=0, tail_split=1, tail_text="")
            if dec != "-":
                r["tail_tiles"], r["tail_split"] = (int(x) for x in dec.split("x"))
                r["tail_text"] = m.group(17) or ""
            out.append(r)
    return out


def test_planner_reproduces_the_golden_tail_table(table):
    with open(GOLDEN) as f:
        want = f.read()
    if table != want:
        diff = "".join(list(difflib.unified_diff(want.splitlines(True), table.splitlines(True), "golden", "planner"))[:80])
        pytest.fail("the planner's tail-split choices differ from tests/golden/gemm_plan_tail.txt:\n" + diff)


def test_case_list_covers_what_the_rule_depends_on(rows):
    assert {r["cus"] for r in rows} == {256, 304, 64}
    assert {r["mode"] for r in rows} == {0, 1, 2, 4, 16}
    assert {r["fsplit"] for r in rows} == {-1, 0, 2}
    assert {r["strict"] for r in rows} == {0, 1}
    assert {r["forced"] for r in rows} == {-1, 6, 7, 9}
    assert {r["tile"] for r in rows if r["tail_tiles"]} == {1, 2, 3}, "a tail split on every K-split tile"
    assert {(r["variant"], r["forced"] < 0) for r in rows if r["tail_tiles"]} >= {(6, True), (6, False), (7, False), (9, False)}
    with open(os.path.join(ROOT, "tests", "golden", "benchmark_configs.json")) as f:
        cfg = json.load(f)
    want = {(c["batch"], c["layers"][1], c["layers"][0], bool(c["bias"])) for fam in ("matmul", "fc") for c in cfg[fam] if c["float_type"] == "f32"}
    assert len(want) == 34
    have = {(r["m"], r["n"], r["k"], "B" in r["ep"]) for r in rows if r["forced"] == -1}
    assert want <= have, want - have
    for shape in ((1024, 1536, 1024), (1024, 1280, 1024)):
        assert any((r["m"], r["n"], r["k"]) == shape for r in rows)
    for tile in (1, 2, 3):  # a 272-tile shape per tile, and chunk counts on both sides of chunks / 4 and of the saving threshold
        assert any(r["tiles"] == 272 and r["tile"] == tile and r["tail_tiles"] == 16 for r in rows if r["cus"] == 256)
        m1 = [r for r in rows if r["mode"] == 1 and r["fsplit"] == -1 and r["cus"] == 256 and r["tile"] == tile and r["launcher"] == "f32_lw"
              and r["tiles"] > 256 and 0 < r["tiles"] % 256 <= 128]
        assert any(r["tail_tiles"] for r in m1) and any(not r["tail_tiles"] and r["chunks"] < 8 for r in m1)
        # (64x64 + K2: 0.92 us per chunk - eight chunks, the least that chunks / 4 lets through, already save more than the hand-off)
        assert tile == 1 or any(not r["tail_tiles"] and r["chunks"] >= 8 for r in m1), "eligible by chunks / 4, refused by the saving test"


def test_every_line_keeps_the_rule(rows):
    chosen = 0
    for r in rows:
        if r["mode"] == 0 or r["fsplit"] >= 0:
            # off, or a forced split count: today's decision, field by field (the driver's "-")
            assert (r["tail_tiles"], r["tail_split"]) == (0, 1), r["line"]
        if not r["tail_tiles"]:
            assert r["tail_split"] == 1, r["line"]
            continue
        chosen += 1
        cus, tiles, S, chunks, tail = r["cus"], r["tiles"], r["tail_split"], r["chunks"], r["tail_tiles"]
        assert r["launcher"] == "f32_lw" and r["tile"] in (1, 2, 3) and r["split"] == 1 and r["text"] == "", r["line"]
        assert r["tail_text"].startswith("brgemm_f32_lw<") and r["tail_text"].endswith(", tail split"), r["line"]
        assert tiles > cus, r["line"]
        assert 0 < tail <= cus // 2, r["line"]
        assert (tiles - tail) % cus == 0 and (tiles - tail) // cus == tiles // cus >= 1, r["line"]
        assert tail * S <= cus, r["line"]
        assert 2 <= S <= 16, r["line"]
        assert S <= chunks, r["line"]
        if r["mode"] == 1:
            assert S <= chunks // 4, r["line"]
            assert S == min(cus // tail, 16, chunks // 4), r["line"]
        else:
            assert S == min(r["mode"], 16, chunks), r["line"]
    assert chosen > 50


def test_the_reference_shapes_get_the_expected_tail(rows):
    def pick(m, n, k, forced, ep="b"):
        got = [r for r in rows if (r["m"], r["n"], r["k"], r["forced"], r["ep"], r["cus"], r["mode"], r["fsplit"], r["strict"]) ==
               (m, n, k, forced, ep, 256, 1, -1, 0)]
        assert got
        return {(r["tail_tiles"], r["tail_split"], r["tail_text"]) for r in got}
    want = {(128, 2, "brgemm_f32_lw<64x64,k2>, tail split")}
    assert pick(1024, 2560, 1024, -1) == want        # 640 tiles of 64x64: 2.5 rounds, br 16
    assert pick(1024, 2560, 1024, -1, "bBr") == want
    assert pick(1024, 2560, 1024, -1, "-") == want
    assert pick(1024, 1536, 1024, 6) == want         # 384 tiles: 1.5 rounds (as planned it runs on 128x64 tiles: one round)
    # strict mode takes the same decision: it depends on the descriptor, the batch count and the CU count only
    strict = [r for r in rows if (r["m"], r["n"], r["k"], r["forced"], r["cus"], r["mode"], r["strict"], r["fsplit"]) ==
              (1024, 2560, 1024, -1, 256, 1, 1, -1)]
    assert strict and all((r["tail_tiles"], r["tail_split"]) == (128, 2) for r in strict)
