"""CPU regression of the planner under the skinny split switch (tpp-mlir_amd/csrc/gemm_plan.cpp plan_gemm_call, xsmm_hip_set_skinny_split):
tests/gemm_plan_skinny_split/driver.cpp steps whole-layer calls - the three B images x m in {1, 16, 17, 31, 32} x n in {16, 200, 1024, 4096} x
(k, br) in {(32, 1), (64, 16), (64, 64), (1000, 1)}, and an f32 call, a forced generic kernel and beta 1 - through plan_gemm and
plan_gemm_call under skinny modes 0, 1 and 32 x split modes 0, 1, 3 and 16 at 64, 256 and 304 compute units, strict mode off and on, alone
and with every other switch on. tests/golden/gemm_plan_skinny_split.txt is the reviewed table; the rule is restated here from the
header's contract text, and the cells of split mode 0 are checked against tests/golden/gemm_plan_skinny.txt wherever that table has the
call."""
import difflib
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tpp-mlir_amd", "csrc")
GOLDEN = os.path.join(ROOT, "tests", "golden", "gemm_plan_skinny_split.txt")
SKINNY_GOLDEN = os.path.join(ROOT, "tests", "golden", "gemm_plan_skinny.txt")
sys.path.insert(0, os.path.join(ROOT, "tpp-mlir_amd"))
import build  # noqa: E402

DESC = re.compile(r"^(v2|v4|flat|f32) (\d+)x(\d+)x(\d+) e(\S+) f(-?\d+) : (\d+) (\S+)$")
CALL = re.compile(r"^ c br(\d+) : (.*?) \| 0: (.*) \| 1: (.*) \| 32: (.*)$")
VFAC = {"v2": 2, "v4": 4, "flat": 1}
MS, NS, KBR = (1, 16, 17, 31, 32), (16, 200, 1024, 4096), ((32, 1), (64, 16), (64, 64), (1000, 1))
CUS = (64, 256, 304)
SPLITS = (0, 1, 3, 16)
V_GENERIC = 8


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    try:
        cc = build.hipcc()
    except RuntimeError as e:
        pytest.fail(str(e))
    d = tmp_path_factory.mktemp("gemm_plan_skinny_split")
    objs = []
    for src, name in ((os.path.join(CSRC, "gemm_plan.cpp"), "gemm_plan.o"), (os.path.join(ROOT, "tests", "gemm_plan_skinny_split", "driver.cpp"), "driver.o")):
        obj = str(d / name)
        subprocess.check_call([cc] + build.FLAGS + ["-x", "hip", "-I" + CSRC, "-c", src, "-o", obj])
        objs.append(obj)
    exe = str(d / "plan_skinny_split")
    subprocess.check_call([cc, "--offload-arch=" + build.ARCH] + objs + ["-o", exe])
    return subprocess.run([exe], capture_output=True, text=True, check=True, timeout=300).stdout


def groups(block):
    """'a b c / d e f / ..' -> {split mode: (cell at 64, 256, 304 CUs)}"""
    g = [tuple(x.split()) for x in block.split(" / ")]
    assert len(g) == 4 and all(len(x) == 3 for x in g), block
    return dict(zip(SPLITS, g))


@pytest.fixture(scope="module")
def rows(table):
    out, desc = [], None
    for l in table.splitlines():
        m = DESC.match(l)
        if m:
            g = m.groups()
            desc = dict(form=g[0], m=int(g[1]), n=int(g[2]), k=int(g[3]), ep=g[4], forced=int(g[5]), variant=int(g[6]), desc_line=l)
            continue
        c = CALL.match(l)
        assert c and desc, "unreadable line (a '!' marks a violated invariant): " + l
        g = c.groups()
        out.append(dict(desc, br=int(g[0]), m0=g[1], cells={0: groups(g[2]), 1: groups(g[3]), 32: groups(g[4])}, line=desc["desc_line"] + " /" + l))
    return out


def test_planner_reproduces_the_golden_table(table):
    with open(GOLDEN) as f:
        want = f.read()
    if table != want:
        diff = "".join(list(difflib.unified_diff(want.splitlines(True), table.splitlines(True), "golden", "planner"))[:80])
        pytest.fail("the planner's choices under xsmm_hip_set_skinny_split differ from tests/golden/gemm_plan_skinny_split.txt:\n" + diff)


def test_no_line_marks_a_violated_invariant(table):
    """the driver's own checks: split mode 0 is an environment that never names the field, strict mode gives the same answer, a forcing
    split mode does not read the compute units, no other switch changes this one, with the skinny switch off the split mode changes
    nothing, and a split launch is the skinny launch of split mode 0 with split > 1 and "_split" in its text - field by field"""
    assert "!" not in table, [l for l in table.splitlines() if "!" in l][:5]


def test_the_table_has_the_whole_sweep(rows):
    for form in VFAC:
        got = {(r["m"], r["n"], r["k"], r["br"]) for r in rows if r["form"] == form and r["forced"] == -1 and r["ep"] == "bBr"}
        assert {(m, n, k, br) for m in MS for n in NS for k, br in KBR} == got
    assert {r["form"] for r in rows} == {"v2", "v4", "flat", "f32"}
    assert any(r["forced"] == V_GENERIC for r in rows) and any(r["ep"] == "-" for r in rows)


def test_split_mode_0_is_the_skinny_golden(rows):
    """with split mode 0 every answer is that of tests/golden/gemm_plan_skinny.txt: the mode-0 launch, the rule's cells and the cell of BN
    32, for every call the two sweeps share"""
    from test_gemm_plan_skinny import CALL as SCALL, DESC as SDESC
    want, key = {}, None
    with open(SKINNY_GOLDEN) as f:
        for l in f.read().splitlines():
            m = SDESC.match(l)
            if m:
                g = m.groups()
                key = (g[0], int(g[1]), int(g[2]), int(g[3]), g[7], int(g[8])) if not g[4] else None
                continue
            c = SCALL.match(l)
            if c and key and not c.group(2):
                want[key + (int(c.group(1)),)] = (c.group(5), c.groups()[5:8], c.group(10))
    shared = 0
    for r in rows:
        w = want.get((r["form"], r["m"], r["n"], r["k"], r["ep"], r["forced"], r["br"]))
        if w:
            shared += 1
            assert (r["m0"], r["cells"][1][0], r["cells"][32][0][1]) == w, r["line"]
            assert len(set(r["cells"][32][0])) == 1 and set(r["cells"][0][0]) == {"-"}, r["line"]
    assert shared >= 3 * 5 * 3 * 3  # (n, k, br) in {16, 1024, 4096} x {(32, 1), (64, 16), (1000, 1)}


def steps(r):
    return r["br"] * -(-r["k"] // 32)


def skinny_bn(cell):
    """'S16x32' -> 32; '-' -> 0"""
    return int(cell.split("x")[1]) if cell.startswith("S") else 0


def rule_parts(r, bn, cus):
    """mode 1, restated from the contract text: 4 parts, else 2, where the parts fit the compute units in one round and a part keeps at
    least 128 KiB of B"""
    blocks = -(-r["n"] // bn)
    for c in (4, 2):
        if blocks * c <= cus and 2 * bn * r["br"] * r["k"] >= c * (128 << 10):
            return c
    return 1


def test_every_row_keeps_the_rule(rows):
    taken = {1: 0, 3: 0, 16: 0}
    for r in rows:
        assert "skinny" not in r["m0"], r["line"]
        for sm in (0, 1, 32):
            base = r["cells"][sm][0]
            for P in (1, 3, 16):
                for cu, skinny, cell in zip(CUS, base, r["cells"][sm][P]):
                    bn = skinny_bn(skinny)
                    if not bn:  # not on the skinny kernel: the split mode changes nothing
                        assert cell == "-", (sm, P, r["line"])
                        continue
                    want = rule_parts(r, bn, cu) if P == 1 else P
                    pe = min(want, steps(r))  # split == P_eff wherever the split is taken
                    assert cell == ("P%d" % pe if pe >= 2 else "-"), (sm, P, cu, r["line"])
                    taken[P] += pe >= 2
    assert taken[3] > 500 and taken[16] > 500 and taken[1] >= 20, taken


def test_what_is_never_split(rows):
    for r in rows:
        never = r["form"] == "f32" or r["m"] >= 32 or r["forced"] != -1 or steps(r) < 2
        if never:
            assert all(set(r["cells"][sm][P]) == {"-"} for sm in (0, 1, 32) for P in (1, 3, 16)), r["line"]
        assert all(set(r["cells"][0][P]) == {"-"} for P in SPLITS), r["line"]  # the skinny switch off


def test_the_measured_rows(rows):
    """profiles/skinny_split_ab.txt: the rows that decided mode 1, as K = br x k, at 256 compute units"""
    def pick(form, m, n, k, br, sm=1):
        got = {(r["cells"][sm][0][1], r["cells"][sm][1][1]) for r in rows if (r["form"], r["m"], r["n"], r["k"], r["br"]) == (form, m, n, k, br) and r["forced"] == -1 and r["ep"] == "bBr"}
        assert len(got) == 1, (form, m, n, k, br, got)
        return got.pop()
    for m in (1, 16):
        assert pick("v2", m, 4096, 64, 64) == ("S16x32", "P2")      # 4096 x 4096: 256 KiB a block, 128 blocks
        assert pick("flat", m, 4096, 64, 64) == ("S16x64", "P4")    # 512 KiB a block, 64 blocks
        assert pick("v4", m, 4096, 64, 64) == ("S16x16", "-")       # 128 KiB a block, 256 blocks
        assert pick("v2", m, 1024, 64, 64) == ("S16x16", "-")       # 1024 x 4096 on BN 16: 128 KiB a block - mixed, not taken
        assert pick("v2", m, 1024, 64, 64, 32) == ("S16x32", "P2")  # ... on BN 32: 256 KiB a block, 32 blocks
        assert pick("v2", m, 1024, 64, 16) == ("S16x16", "-") and pick("v2", m, 4096, 64, 16) == ("S16x16", "-")  # K = 1024: every P lost
        assert pick("v2", m, 1024, 1000, 1) == ("S16x16", "-")
    assert pick("v2", 31, 4096, 64, 64) == ("-", "-")               # the skinny switch's gate stays that switch's
    assert pick("v2", 31, 4096, 64, 64, 32) == ("S32x32", "P2")
