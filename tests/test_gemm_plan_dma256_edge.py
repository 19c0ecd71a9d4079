"""CPU regression of the planner under the edge tiles of the 256x256 bf16 tile (tpp-mlir_amd/csrc/gemm_plan.cpp plan_gemm_call,
xsmm_hip_set_dma256_edge): tests/gemm_plan_dma256_edge/driver.cpp steps whole-layer bf16 calls - the three B images x the measured shapes of
profiles/dma256_edge_ab.txt, a divisible 256 x 256, m = 255 and n = 248 (below the tile), n = 4004 (n % 8), k = 1000 (k % 32), k = 96 (k %
64, taken), 240 and 225 tiles (the rule's edge), rows of tests/golden/gemm_plan.txt, each misalignment, beta 1, wide and off-grid leading
dimensions, forced variants, the generic kernel forced, a VNNI C, batch count 0, strict mode - through plan_gemm and plan_gemm_call under
modes 0, 1 and 2. tests/golden/gemm_plan_dma256_edge.txt is the reviewed table; the rule is restated here from the issue."""
import difflib
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tpp-mlir_amd", "csrc")
GOLDEN = os.path.join(ROOT, "tests", "golden", "gemm_plan_dma256_edge.txt")
PLAN = os.path.join(ROOT, "tests", "golden", "gemm_plan.txt")
sys.path.insert(0, os.path.join(ROOT, "tpp-mlir_amd"))
import build  # noqa: E402

DESC = re.compile(r"^(v2|v4|flat|vc|vc4) (\d+)x(\d+)x(\d+)(?: ld(\d+),(\d+),(\d+))? e(\S+) f(-?\d+) : (\d+) (\S+)( gf)?( vf)?(?: bk(\d))?$")
CALL = re.compile(r"^ c br(\d+)(?: a(\d+)/(\d+)/(\d+))?( strict)? : (.*) \| (.*) \| (.*) \| others (\w+)$")
KIND = {"v2": 0, "flat": 2, "v4": 4}
TEXT = {0: 'bf16_fast t2 b0 edge "brgemm_bf16_dma<256x256>, edge tiles"', 2: 'bf16_fast t2 b2 edge "brgemm_bf16_dma_flatb<256x256>, edge tiles"',
        4: 'bf16_fast t2 b4 edge "brgemm_bf16_dma_vnni4<256x256>, edge tiles"'}
MEASURED = [(4000, 4096, 1024), (4096, 4000, 1024), (4100, 4096, 1024), (5000, 5000, 1024), (8000, 8000, 1024), (16000, 1024, 1024)]


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    try:
        cc = build.hipcc()
    except RuntimeError as e:
        pytest.fail(str(e))
    d = tmp_path_factory.mktemp("gemm_plan_dma256_edge")
    objs = []
    for src, name in ((os.path.join(CSRC, "gemm_plan.cpp"), "gemm_plan.o"), (os.path.join(ROOT, "tests", "gemm_plan_dma256_edge", "driver.cpp"), "driver.o")):
        obj = str(d / name)
        subprocess.check_call([cc] + build.FLAGS + ["-x", "hip", "-I" + CSRC, "-c", src, "-o", obj])
        objs.append(obj)
    exe = str(d / "plan_dma256_edge")
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
            desc = dict(form=g[0], m=int(g[1]), n=int(g[2]), k=int(g[3]), ld=tuple(int(x) for x in g[4:7]) if g[4] else None, ep=g[7], forced=int(g[8]),
                        variant=int(g[9]), name=g[10], gf=bool(g[11]), vf=bool(g[12]), desc_line=l)
            continue
        c = CALL.match(l)
        assert c and desc, "unreadable line: " + l
        g = c.groups()
        assert "!" not in l, l
        out.append(dict(desc, br=int(g[0]), ab=int(g[1] or 16), c=int(g[2] or 16), d=int(g[3] or 16), strict=bool(g[4]), m0=g[5],
                        m1=g[5] if g[6] == "-" else g[6], m2=g[5] if g[7] == "-" else g[7], others=g[8], call_key=l.split(" : ")[0].strip(),
                        line=desc["desc_line"] + " /" + l))
    return out


def test_planner_reproduces_the_golden_table(table):
    with open(GOLDEN) as f:
        want = f.read()
    if table != want:
        diff = "".join(list(difflib.unified_diff(want.splitlines(True), table.splitlines(True), "golden", "planner"))[:80])
        pytest.fail("the planner's choices under xsmm_hip_set_dma256_edge differ from tests/golden/gemm_plan_dma256_edge.txt:\n" + diff)


def test_the_table_has_every_case(rows):
    shapes = set(MEASURED) | {(256, 256, 1024), (255, 4096, 1024), (4096, 248, 1024), (4096, 4004, 1024), (4000, 4096, 1000), (4000, 4096, 96),
                              (3800, 4096, 1024), (3800, 3800, 1024), (4096, 4096, 4096)}
    for form in ("v2", "v4", "flat"):
        plain = [r for r in rows if r["form"] == form and r["forced"] == -1 and r["ep"] == "b" and not r["ld"]]
        assert {(r["m"], r["n"], r["k"]) for r in plain} == shapes
        for s in shapes:
            assert {(r["br"], r["strict"]) for r in plain if (r["m"], r["n"], r["k"]) == s} == {(1, False), (1, True), (4, False), (0, False)}
        assert {(r["ab"], r["c"], r["d"]) for r in rows if r["form"] == form and r["ep"] == "bBr" and r["m"] == 4000} == {
            (16, 16, 16), (8, 16, 16), (16, 8, 16), (16, 16, 4), (16, 16, 8)}
        assert any(r["vf"] and not r["gf"] for r in rows if r["form"] == form) and any(r["gf"] for r in rows if r["form"] == form)
        assert any(r["ep"] == "-" for r in rows if r["form"] == form) and any(r["ld"] for r in rows if r["form"] == form)
    assert {r["form"] for r in rows} == {"v2", "v4", "flat", "vc", "vc4"}


def test_no_other_switch_changes_this_switchs_decision(rows):
    assert len(rows) > 250 and all(r["others"] == "same" for r in rows), [r["line"] for r in rows if r["others"] != "same"][:5]


def test_strict_mode_changes_no_row(rows):
    n = 0
    for r in rows:
        if r["strict"]:
            twin = [x for x in rows if x["desc_line"] == r["desc_line"] and x["br"] == r["br"] and not x["strict"] and (x["ab"], x["c"], x["d"]) == (16, 16, 16)]
            assert len(twin) == 1 and (twin[0]["m0"], twin[0]["m1"], twin[0]["m2"]) == (r["m0"], r["m1"], r["m2"]), r["line"]
            n += 1
    assert n >= 60 and any(r["strict"] and r["m1"] in TEXT.values() for r in rows), "strict mode takes the switch's decision"


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
    # D8 / D9 / D10: the 4096^3 rows of the three images; D32 / D34: 1024 x 352 x 512, ragged in n and eligible under mode 2
    want = {(f, 4096, 4096, 4096, br) for f in ("v2", "v4", "flat") for br in (1, 0)} | {(f, 1024, 352, 512, 1) for f in ("v2", "v4")}
    assert want <= matched, sorted(matched)


def rule(r, mode):
    """does the call run on the edge tiles of the 256x256 tile - restated from the issue"""
    if mode == 0 or r["form"] not in KIND or r["gf"] or r["vf"]:
        return False
    m, n, k = r["m"], r["n"], r["k"]
    if m < 256 or n < 256 or not (m % 256 or n % 256) or n % 8 or k % 32 or r["br"] < 1:
        return False
    if r["ab"] < 16 or r["c"] < 16 or ("B" in r["ep"] and r["d"] < 8):
        return False
    if r["ld"] and any(x % 8 for x in r["ld"]):
        return False
    if mode == 2:
        return True
    t256, t128 = -(-m // 256) * -(-n // 256), -(-m // 128) * -(-n // 128)
    fill = lambda t: t / (-(-t // 256) * 256)  # noqa: E731
    return t256 >= 240 and 1.4 * fill(t256) >= fill(t128)


def test_every_row_keeps_the_rule(rows):
    taken = {1: 0, 2: 0}
    for r in rows:
        assert "edge tiles" not in r["m0"], r["line"]
        for mode in (1, 2):
            got = r["m%d" % mode]
            if rule(r, mode):
                assert got == TEXT[KIND[r["form"]]], (mode, r["line"])
                taken[mode] += 1
            else:
                assert got == r["m0"], (mode, r["line"])
    assert taken[1] >= 60 and taken[2] > taken[1]


def test_the_named_shapes(rows):
    def pick(form, m, n, k, mode, br=1):
        got = {r["m%d" % mode] for r in rows if (r["form"], r["m"], r["n"], r["k"], r["br"]) == (form, m, n, k, br) and r["forced"] == -1 and r["ep"] == "b"
               and not r["strict"] and not r["ld"]}
        assert len(got) == 1, got
        return got.pop()
    for form, bk in KIND.items():
        # the measured rows: every one that gained is the rule's; 4100 x 4096 (272 tiles, a second round: slower than the 128x128 edge tile) is not
        for m, n, k in MEASURED:
            assert pick(form, m, n, k, 2) == TEXT[bk]
            assert (pick(form, m, n, k, 1) == TEXT[bk]) == ((m, n) != (4100, 4096)), (form, m, n)
        assert pick(form, 3800, 4096, 1024, 1) == TEXT[bk] and pick(form, 3800, 3800, 1024, 1) != TEXT[bk] and pick(form, 3800, 3800, 1024, 2) == TEXT[bk]
        assert pick(form, 4000, 4096, 96, 2) == TEXT[bk]
        for m, n, k in ((256, 256, 1024), (255, 4096, 1024), (4096, 248, 1024), (4096, 4004, 1024), (4000, 4096, 1000), (4096, 4096, 4096)):
            assert "edge tiles" not in pick(form, m, n, k, 2), (form, m, n, k)
        assert "edge tiles" not in pick(form, 4000, 4096, 1024, 2, br=0)
