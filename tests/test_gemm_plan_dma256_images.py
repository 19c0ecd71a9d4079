"""CPU check of the planner's rule for a flat or VNNI-4 B on the 256x256 bf16 tile (tpp-mlir_amd/csrc/gemm_plan.cpp plan_gemm_call,
xsmm_hip_set_dma256_images): tests/gemm_plan_dma256_images/driver.cpp steps whole-layer bf16 calls - the three B images x 4096^3, 4096 x 4096 x
1024, 3840 x 4096 (240 tiles of 256x256: the rule's edge), 3584 x 4096 (224: under it), 16384 x 1024, 256 x 256, 512 x 768, 4100 x 4096,
8192 x 8192, 2048^3, with a bias row and each misalignment, beta 1, wide leading dimensions, forced variants, a VNNI C, batch counts 1, 4 and
0, strict mode - through plan_gemm and plan_gemm_call under modes 0, 1 and 2. tests/golden/gemm_plan_dma256_images.txt is the reviewed
record. Whatever the table says: VNNI-2 rows are the same in all modes; strict mode changes no row; a mode-0 row whose descriptor and call
tests/golden/gemm_plan.txt has too is that table's row; and every row satisfies the rule as restated here from its issue (rule)."""
import difflib
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tpp-mlir_amd", "csrc")
GOLDEN = os.path.join(ROOT, "tests", "golden", "gemm_plan_dma256_images.txt")
PLAN = os.path.join(ROOT, "tests", "golden", "gemm_plan.txt")
sys.path.insert(0, os.path.join(ROOT, "tpp-mlir_amd"))
import build  # noqa: E402

DESC = re.compile(r"^(v2|v4|flat|vc|vc4) (\d+)x(\d+)x(\d+)(?: ld(\d+),(\d+),(\d+))? e(\S+) f(-?\d+) : (\d+) (\S+)( gf)?( vf)?(?: bk(\d))?$")
CALL = re.compile(r"^ c br(\d+)(?: a(\d+)/(\d+)/(\d+))?( strict)? : (.*) \| (.*) \| (.*)$")
TEXT = {2: 'bf16_fast t2 b2 "brgemm_bf16_dma_flatb<256x256>"', 4: 'bf16_fast t2 b4 "brgemm_bf16_dma_vnni4<256x256>"'}


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    try:
        cc = build.hipcc()
    except RuntimeError as e:
        pytest.fail(str(e))
    d = tmp_path_factory.mktemp("gemm_plan_dma256_images")
    objs = []
    for src, name in ((os.path.join(CSRC, "gemm_plan.cpp"), "gemm_plan.o"), (os.path.join(ROOT, "tests", "gemm_plan_dma256_images", "driver.cpp"), "driver.o")):
        obj = str(d / name)
        subprocess.check_call([cc] + build.FLAGS + ["-x", "hip", "-I" + CSRC, "-c", src, "-o", obj])
        objs.append(obj)
    exe = str(d / "plan_dma256_images")
    subprocess.check_call([cc, "--offload-arch=" + build.ARCH] + objs + ["-o", exe])
    return subprocess.run([exe], capture_output=True, text=True, check=True, timeout=120).stdout


@pytest.fixture(scope="module")
def rows(table):
    """one row per call: the descriptor's facts, the call's, and the three launches (modes 1 and 2 resolved: "-" = the mode-0 one)"""
    out, desc = [], None
    for l in table.splitlines():
        m = DESC.match(l)
        if m:
            g = m.groups()
            desc = dict(form=g[0], m=int(g[1]), n=int(g[2]), k=int(g[3]), ep=g[7], forced=int(g[8]), variant=int(g[9]), name=g[10], gf=bool(g[11]),
                        vf=bool(g[12]), bk=int(g[13]) if g[13] else -1, desc_line=l)
            continue
        c = CALL.match(l)
        assert c and desc, "unreadable line: " + l
        g = c.groups()
        assert "!" not in l, l
        out.append(dict(desc, br=int(g[0]), ab=int(g[1] or 16), c=int(g[2] or 16), d=int(g[3] or 16), strict=bool(g[4]), m0=g[5],
                        m1=g[5] if g[6] == "-" else g[6], m2=g[5] if g[7] == "-" else g[7], call_key=l.split(" : ")[0].strip(), line=desc["desc_line"] + " /" + l))
    return out


def test_planner_reproduces_the_golden_table(table):
    with open(GOLDEN) as f:
        want = f.read()
    if table != want:
        diff = "".join(list(difflib.unified_diff(want.splitlines(True), table.splitlines(True), "golden", "planner"))[:80])
        pytest.fail("the planner's choices under xsmm_hip_set_dma256_images differ from tests/golden/gemm_plan_dma256_images.txt:\n" + diff)


def test_the_table_has_every_case(rows):
    shapes = {(4096, 4096, 4096), (4096, 4096, 1024), (3840, 4096, 1024), (3584, 4096, 1024), (16384, 1024, 1024), (256, 256, 1024), (512, 768, 1024),
              (4100, 4096, 1024), (8192, 8192, 1024), (2048, 2048, 2048)}
    for form in ("v2", "v4", "flat"):
        plain = [r for r in rows if r["form"] == form and r["forced"] == -1 and r["ep"] == "b" and " ld" not in r["desc_line"]]
        assert {(r["m"], r["n"], r["k"]) for r in plain} == shapes
        for s in shapes:
            assert {(r["br"], r["strict"]) for r in plain if (r["m"], r["n"], r["k"]) == s} == {(1, False), (1, True), (4, False), (0, False)}
        assert {(r["ab"], r["c"], r["d"]) for r in rows if r["form"] == form and r["ep"] == "bBr"} == {(16, 16, 16), (8, 16, 16), (16, 8, 16), (16, 16, 4), (16, 16, 8)}
        assert any(r["vf"] for r in rows if r["form"] == form) and any(r["ep"] == "-" for r in rows if r["form"] == form)
    assert any(r["gf"] for r in rows if r["form"] in ("v4", "flat")) and {r["form"] for r in rows} == {"v2", "v4", "flat", "vc", "vc4"}


def test_vnni2_rows_are_the_same_in_all_modes(rows):
    v2 = [r for r in rows if r["form"] in ("v2", "vc")]
    assert len(v2) > 50 and all(r["m0"] == r["m1"] == r["m2"] for r in v2)


def test_strict_mode_changes_no_row(rows):
    n = 0
    for r in rows:
        if r["strict"]:
            twin = [x for x in rows if x["desc_line"] == r["desc_line"] and x["br"] == r["br"] and not x["strict"] and (x["ab"], x["c"], x["d"]) == (16, 16, 16)]
            assert len(twin) == 1 and (twin[0]["m0"], twin[0]["m1"], twin[0]["m2"]) == (r["m0"], r["m1"], r["m2"]), r["line"]
            n += 1
    assert n >= 30


def test_mode_0_rows_are_the_rows_of_the_planner_table(rows):
    """tests/golden/gemm_plan.txt numbers its descriptors: a descriptor line there is "D<id> " + ours, a call line "D<id> c ... : <launch>"."""
    with open(PLAN) as f:
        plan = f.read().splitlines()
    ids = {}
    for l in plan:
        m = re.match(r"^D(\d+) ((?:v2|v4|flat|vc) .*)$", l)
        if m:
            ids.setdefault(m.group(2), m.group(1))
    calls = {}
    for l in plan:
        m = re.match(r"^D(\d+) (c br\d+(?: a\d+/\d+/\d+)?(?: strict)?) : (.*)$", l)
        if m:
            calls[(m.group(1), m.group(2))] = m.group(3)
    matched = set()
    for r in rows:
        key = (ids.get(r["desc_line"]), r["call_key"])
        if key in calls:
            assert calls[key] == r["m0"], (r["line"], calls[key])
            matched.add((r["form"], r["m"], r["n"], r["k"], r["br"]))
    # D8 / D9 / D10: the 4096^3 rows of the three images, one batch element and none
    assert {(f, 4096, 4096, 4096, br) for f in ("v2", "v4", "flat") for br in (1, 0)} <= matched, sorted(matched)


def rule(r, mode):
    """does the call go to the 256x256 tile with its image - restated from the issue"""
    if mode == 0 or r["form"] not in ("v4", "flat") or r["gf"] or r["vf"] or not 24 <= r["variant"] <= 31 or r["bk"] not in (2, 4):
        return False
    if r["m"] % 256 or r["n"] % 256 or r["br"] < 1 or r["ab"] < 16 or r["c"] < 16 or ("B" in r["ep"] and r["d"] < 8):
        return False
    if mode == 2:
        return True
    t256, t128 = (r["m"] // 256) * (r["n"] // 256), (r["m"] // 128) * (r["n"] // 128)
    fill = lambda t: t / (-(-t // 256) * 256)  # noqa: E731
    return t256 >= 240 and 1.4 * fill(t256) >= fill(t128)


def test_every_row_keeps_the_rule(rows):
    taken = {1: 0, 2: 0}
    for r in rows:
        for mode in (1, 2):
            got = r["m%d" % mode]
            if rule(r, mode):
                assert got == TEXT[r["bk"]], (mode, r["line"])
                taken[mode] += 1
            else:
                assert got == r["m0"], (mode, r["line"])
        assert "256x256>\"" not in r["m0"] or r["form"] == "v2", r["line"]
    assert taken[1] >= 40 and taken[2] > taken[1]


def test_the_named_shapes(rows):
    def pick(form, m, n, k, mode, br=1):
        got = {r["m%d" % mode] for r in rows if (r["form"], r["m"], r["n"], r["k"], r["br"]) == (form, m, n, k, br) and r["forced"] == -1 and r["ep"] == "b"
               and not r["strict"] and " ld" not in r["desc_line"]}
        assert len(got) == 1, got
        return got.pop()
    for form, bk in (("flat", 2), ("v4", 4)):
        for m, n, k in ((4096, 4096, 4096), (3840, 4096, 1024), (16384, 1024, 1024)):
            assert pick(form, m, n, k, 1) == TEXT[bk] and pick(form, m, n, k, 2) == TEXT[bk]
        assert pick(form, 3584, 4096, 1024, 1) == "bf16_lw t3 b%d" % bk and pick(form, 3584, 4096, 1024, 2) == TEXT[bk]
        assert pick(form, 2048, 2048, 2048, 1) == "bf16_lw t3 b%d" % bk and pick(form, 2048, 2048, 2048, 2) == TEXT[bk]
        assert pick(form, 256, 256, 1024, 2) == TEXT[bk] and pick(form, 512, 768, 1024, 2) == TEXT[bk] and "256x256" not in pick(form, 256, 256, 1024, 1)
        assert "generic" in pick(form, 4100, 4096, 1024, 2) and "generic" in pick(form, 4096, 4096, 4096, 2, br=0)
