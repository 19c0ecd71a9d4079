"""CPU check of the planner's ragged mixed-width chain rule (tpp-mlir_amd/csrc/gemm_plan.cpp plan_chain_widths_ragged and
chain_widths_ragged_b_kind, xsmm_hip_set_chain_widths_ragged): tests/gemm_plan_chain_widths_ragged/driver.cpp, compiled with the library's
flags, steps layer chains - the rows of the A/B at 256, 64 and 304 compute units, the GPU test's chains with every edge tile forced and the
three B images, the partition against the three existing chain rules, strict mode, a forced tile without an instance, and one refusal each -
through the rule the way try_chain_launch asks it. One line per chain and CU count; tests/golden/gemm_plan_chain_widths_ragged.txt is the
reviewed record. Whatever the table says, every line must also satisfy the rule as restated here from its issue; every refusal is reached;
no chain is taken by both this rule and plan_chain_widths; and tests/golden/gemm_plan.txt is what it was."""
import difflib
import hashlib
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tpp-mlir_amd", "csrc")
GOLDEN = os.path.join(ROOT, "tests", "golden", "gemm_plan_chain_widths_ragged.txt")
sys.path.insert(0, os.path.join(ROOT, "tpp-mlir_amd"))
import build  # noqa: E402

LINE = re.compile(r'^(\d+) n([\d,]+) k([\d,]+) br([\d,]+) (f32|bf16) vf(\d) f(-?\d+) sw([01]) et(-?\d) st([01]) x(\d+) cus(\d+) : kind(-?\d) "([^"]*)" \| tile(-?\d) g([01]) "([^"]*)"'
                  r' \| widths tile(-?\d) "([^"]*)"(?: \| edge tile(-?\d) "([^"]*)" \| ragged tile(-?\d) "([^"]*)")?$')
TILE = [(32, 64), (64, 64), (64, 128), (128, 128)]
WHYS = ["ragged mixed-width chains are off", "strict mode", "fewer than 2 or more than 8 calls", "do not share one B image", "k below 64 or not a multiple of 8, or an empty batch",
        "an n that is not a multiple of 8", "every call has the same n", "a tile divides m, every n and every k entirely", "below every tile", "more tiles than compute units", "gate: "]
KIND_WHYS = ["ragged mixed-width chains are off", "an f32 call", "stores a VNNI C or is not beta 0", "a forced kernel", "k below 64 or not a multiple of 8", "off the grid",
             "differ in kind"]


def ceil_div(a, b):
    return -(-a // b)


def instance(t, kind):
    return not (t == 2 and kind == 0)


def rule(m, ns, ks, brs, cus, kind, et, strict=False, sw=1):
    """(tile, gated) a ragged mixed-width chain takes, (None, False) = refused - restated from the issue. 2 .. 8 bf16 calls with one B image,
    at least two different n, every k >= 64 and k % 8 == 0, every batch >= 1, every n % 8 == 0, not strict; never a chain some tile divides
    entirely. A tile fits when m >= BM, every n >= BN, its instance exists and ceil(m / BM) * max ceil(n / BN) <= CUs. The forced edge tile if
    it fits, else the smallest that fits; without a forced tile gated where some layer alone fits a smaller tile than the launch's."""
    if not sw or strict or not 2 <= len(ns) <= 8 or kind not in (0, 2, 4) or any(k < 64 or k % 8 for k in ks) or any(b < 1 for b in brs) or any(n % 8 for n in ns) or len(set(ns)) == 1:
        return None, False
    holds = lambda t, widths: m >= TILE[t][0] and all(n >= TILE[t][1] for n in widths)
    if any(holds(t, ns) and m % TILE[t][0] == 0 and all(n % TILE[t][1] == 0 for n in ns) and all(k % 64 == 0 for k in ks) for t in range(4)):
        return None, False  # the partition: the mixed-width rule's
    fit = lambda t, widths: holds(t, widths) and instance(t, kind) and ceil_div(m, TILE[t][0]) * ceil_div(max(widths), TILE[t][1]) <= cus
    fits = [t for t in range(4) if fit(t, ns)]
    if not fits:
        return None, False
    if et in fits:
        return et, False
    tile = fits[0]
    if et < 0 and any(fit(s, [n]) for n in ns for s in range(tile)):
        return tile, True
    return tile, False


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    try:
        cc = build.hipcc()
    except RuntimeError as e:
        pytest.fail(str(e))
    d = tmp_path_factory.mktemp("gemm_plan_chain_widths_ragged")
    objs = []
    for src, name in ((os.path.join(CSRC, "gemm_plan.cpp"), "gemm_plan.o"), (os.path.join(ROOT, "tests", "gemm_plan_chain_widths_ragged", "driver.cpp"), "driver.o")):
        obj = str(d / name)
        subprocess.check_call([cc] + build.FLAGS + ["-x", "hip", "-I" + CSRC, "-c", src, "-o", obj])
        objs.append(obj)
    exe = str(d / "plan_chain_widths_ragged")
    subprocess.check_call([cc, "--offload-arch=" + build.ARCH] + objs + ["-o", exe])
    return subprocess.run([exe], capture_output=True, text=True, check=True, timeout=120).stdout


@pytest.fixture(scope="module")
def rows(table):
    out = []
    names = "m ns ks brs dt vf forced sw et strict extra cus kind kwhy tile gated why wtile wwhy etile ewhy gtile gwhy".split()
    for l in table.splitlines():
        m = LINE.match(l)
        assert m, "unreadable line: " + l
        r = dict(zip(names, m.groups()))
        for k in r:
            if k in ("ns", "ks", "brs"):
                r[k] = [int(x) for x in r[k].split(",")]
            elif k not in ("dt", "why", "kwhy", "wwhy", "ewhy", "gwhy") and r[k] is not None:
                r[k] = int(r[k])
        r["line"] = l
        out.append(r)
    return out


def test_planner_reproduces_the_golden_table(table):
    with open(GOLDEN) as f:
        want = f.read()
    if table != want:
        diff = "".join(list(difflib.unified_diff(want.splitlines(True), table.splitlines(True), "golden", "planner"))[:80])
        pytest.fail("the planner's ragged mixed-width choices differ from tests/golden/gemm_plan_chain_widths_ragged.txt:\n" + diff)


def test_every_line_keeps_the_rule(rows):
    chosen = 0
    for r in rows:
        tile, gated = rule(r["m"], r["ns"], r["ks"], r["brs"], r["cus"], r["kind"], r["et"], bool(r["strict"]), r["sw"])
        assert (r["tile"], r["gated"]) == (-1 if tile is None else tile, int(gated)), ((tile, gated), r["line"])
        assert (r["tile"] >= 0 and not r["gated"]) == (r["why"] == ""), r["line"]
        if r["tile"] >= 0 and not r["gated"]:
            chosen += 1
            bm, bn = TILE[r["tile"]]
            assert r["m"] >= bm and all(n >= bn and n % 8 == 0 for n in r["ns"]) and ceil_div(r["m"], bm) * ceil_div(max(r["ns"]), bn) <= r["cus"], r["line"]
            assert r["m"] % bm or any(n % bn for n in r["ns"]) or any(k % 64 for k in r["ks"]), "something is ragged on the tile: " + r["line"]
            assert r["dt"] == "bf16" and len(set(r["ns"])) > 1 and instance(r["tile"], r["kind"]) and not r["strict"], r["line"]
        if r["kind"] >= 0 and not r["extra"] and r["kwhy"] == "" and r["brs"][0] > 0 and all(k % 8 == 0 and k >= 64 for k in r["ks"]) and all(n % 8 == 0 for n in r["ns"]):
            # what try_chain_launch hands the rule: one B image on every call, no forced kernel
            assert r["dt"] == "bf16" and r["forced"] == -1 and r["kind"] == {2: 0, 0: 2, 4: 4}[r["vf"]], r["line"]
    assert chosen > 100


def test_no_chain_is_taken_by_this_rule_and_the_mixed_width_rule(rows):
    """the partition depends on the descriptors only: a chain some tile divides entirely is never this rule's, whatever the compute units say,
    and what this rule takes the mixed-width rule refuses as ragged"""
    both = [r["line"] for r in rows if r["tile"] >= 0 and r["wtile"] >= 0]
    assert not both, both
    divided = [r for r in rows if "a tile divides m, every n and every k entirely" in r["why"]]
    assert len(divided) >= 5 and any(r["wtile"] >= 0 for r in divided) and any("more tiles than compute units" in r["wwhy"] for r in divided) and any(r["wwhy"].startswith("gate: ") for r in divided)
    for r in rows:
        if r["tile"] >= 0:
            assert "no tile divides m and every n" in r["wwhy"] or "k not in 64-k chunks" in r["wwhy"], r["line"]


def test_equal_widths_are_the_other_three_switches(rows):
    eq = [r for r in rows if r["etile"] is not None]
    assert len(eq) == 8 and all(r["tile"] == -1 and "every call has the same n" in r["why"] and r["wtile"] == -1 for r in eq)
    assert any(r["etile"] >= 0 for r in eq) and any(r["gtile"] >= 0 for r in eq), "the ragged-m and the ragged-width rule still take their chains"


def test_every_refusal_is_reached_and_the_case_list_covers_what_the_issue_names(rows):
    for w in WHYS:
        assert any(w in r["why"] for r in rows), w
    assert all(any(w in r["why"] for w in WHYS) for r in rows if r["tile"] < 0 or r["gated"]), "a why the test does not know"
    for w in KIND_WHYS:
        assert any(w in r["kwhy"] for r in rows), w
    assert {r["cus"] for r in rows} == {64, 256, 304}

    def pick(m, layers, cus=256, vf=2, et=-1, sw=1, strict=0):
        got = [r for r in rows if (r["m"], r["ns"], r["ks"], r["cus"], r["vf"], r["et"], r["sw"], r["strict"]) == (m, layers[1:], layers[:-1], cus, vf, et, sw, strict) and
               all(b == 1 for b in r["brs"]) and r["dt"] == "bf16" and not r["extra"] and r["forced"] == -1 and (r["kwhy"] == "" or not sw)]
        assert got and len({(g["tile"], g["gated"]) for g in got}) == 1, (m, layers, cus, len(got))
        return got[0]
    # the A/B's rows on 256 CUs: taken on the 32x64 tile; the widening chain gated; n = 500 has no image and is refused
    for m, layers in ((1024, [784, 512, 256, 128]), (1000, [784, 512, 256, 128]), (1000, [1024, 512, 256, 128]), (512, [784, 256, 64, 256, 784]), (1000, [1000, 504, 248]),
                      (200, [200, 136, 72, 200])):
        p = pick(m, layers)
        assert (p["tile"], p["gated"]) == (0, 0), (m, layers, p["line"])
    p = pick(1000, [1000, 2000, 1000])
    assert (p["tile"], p["gated"]) == (3, 1) and p["why"].startswith("gate: ")
    assert [(pick(1000, [1000, 2000, 1000], et=t)["tile"], pick(1000, [1000, 2000, 1000], et=t)["gated"]) for t in range(4)] == [(3, 0)] * 4, "forced: no tile but 128x128 fits, not gated"
    n500 = [r for r in rows if r["ns"] == [500, 250]]
    assert n500 and all(r["tile"] == -1 for r in n500) and any("an n that is not a multiple of 8" in r["why"] for r in n500)
    p = pick(1000, [784, 512, 256, 128], cus=64)  # (on 64 CUs only 128x128 fits, and every layer alone fits a smaller tile)
    assert (p["tile"], p["gated"]) == (3, 1) and pick(1000, [784, 512, 256, 128], cus=304)["tile"] == 0
    assert pick(1000, [784, 512, 256, 128], vf=0)["tile"] == 0 and pick(1000, [784, 512, 256, 128], vf=4)["tile"] == 0
    # the GPU test's chains: every tile and image forced, taken on that tile - but 64x128 with VNNI-2, which has no instance: the smallest tile
    for t, (bm, bn) in enumerate(TILE):
        for vf, kind in ((2, 0), (0, 2), (4, 4)):
            for m in (bm + 8, 3 * bm - 3):
                mine = [r for r in rows if r["et"] == t and r["m"] == m and r["vf"] == vf and not r["strict"] and r["sw"] and min(r["ns"]) >= bn and
                        r["ns"][0] in (3 * bn + 8, bn + 8, 4 * bn, 2 * bn, 2 * bn + 8, 2 * bn + 16, 3 * bn) and r["ks"][0] in (192, 128, 72, 200, 136, 144)]
                want = 0 if (t, kind) == (2, 0) else t
                assert len(mine) >= 7 and all((r["tile"], r["gated"]) == (want, 0) for r in mine), (t, vf, m, [r["line"] for r in mine])
                assert any(len(r["ns"]) == 8 for r in mine) and any(r["brs"] == [2, 2, 2] for r in mine) and any(r["brs"] == [3, 1] for r in mine)
    # the GPU test's MLPs under set_edge_tiles(21): taken on 64x64, not with the switch off
    for m, layers in ((200, [200, 136, 72, 200]), (96, [784, 256, 128, 64])):
        assert pick(m, layers, et=1)["tile"] == 1 and pick(m, layers, et=1, sw=0)["tile"] == -1
    # strict mode: never, forced tile or not
    strict = [r for r in rows if r["strict"]]
    assert len(strict) == 2 and all(r["tile"] == -1 and "strict mode" in r["why"] for r in strict) and {r["et"] for r in strict} == {-1, 0}
    # a forced tile without an instance is passed over; the same chain with the flat image takes it
    assert pick(200, [200, 264, 136], et=2)["tile"] == 0 and pick(200, [200, 264, 136], et=2, vf=0)["tile"] == 2
    assert any(len(r["ns"]) == 8 and r["tile"] >= 0 for r in rows) and any(len(r["ns"]) == 9 for r in rows) and any(len(r["ns"]) == 1 for r in rows)


def test_the_single_call_table_is_what_it_was():
    with open(os.path.join(ROOT, "tests", "golden", "gemm_plan.txt"), "rb") as f:
        assert hashlib.sha256(f.read()).hexdigest() == "47d83170a9e065ad7cac7e1f262fe123749fee1f26741562852271ccc04fc960"
