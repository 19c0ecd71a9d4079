"""The gfx950 code object of tpp-mlir_amd/csrc/brgemm_bf16_lw.hip as the compiler reports it: one device-only compile with
-Rpass-analysis=kernel-resource-usage (about 75 s) shared by every test that asks - once per test session, and kept under the temporary
directory, keyed by the newest modification time of the file and the project headers next to it, for the sessions after it.
report() returns {kernel symbol: (scratch bytes per lane, VGPRs, AGPRs)}. And the launch table the instances come from
(tpp-mlir_amd/csrc/brgemm_bf16_lw_launch.h) as tests/blw_launch_table/driver.cpp prints it: launch_table(). A plain module, not a conftest."""
import atexit
import glob
import os
import re
import shutil
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tpp-mlir_amd", "csrc")
SRC = os.path.join(CSRC, "brgemm_bf16_lw.hip")
_report = None
_driver = None


def _parse(text):
    names = re.findall(r"Function Name: (\S+)", text)
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", text)]
    vgprs = [int(x) for x in re.findall(r" VGPRs: (\d+)", text)]
    agprs = [int(x) for x in re.findall(r"AGPRs: (\d+)", text)]
    assert len(names) == len(scratch) == len(vgprs) == len(agprs) == len(set(names)), (len(names), len(scratch), len(vgprs), len(agprs))
    return {n: (s, v, a) for n, s, v, a in zip(names, scratch, vgprs, agprs)}


def report():
    global _report
    if _report is not None:
        return _report
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    assert os.path.exists(hipcc), "needs hipcc"
    stamp = max(os.stat(f).st_mtime_ns for f in [SRC] + glob.glob(os.path.join(CSRC, "*.h")))
    cache = os.path.join(tempfile.gettempdir(), "blw_codeobj_%d" % os.getuid(), "%d.txt" % stamp)
    if os.path.exists(cache):
        with open(cache) as f:
            _report = _parse(f.read())
        return _report
    with tempfile.TemporaryDirectory() as tmp:
        r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-c", SRC, "-o", os.path.join(tmp, "k.o"),
                            "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    _report = _parse(r.stderr)
    os.makedirs(os.path.dirname(cache), exist_ok=True)
    with tempfile.NamedTemporaryFile("w", dir=os.path.dirname(cache), delete=False) as f:
        f.write(r.stderr)
    os.replace(f.name, cache)
    return _report


def launch_table(lines=()):
    """(instances, answers): the instances the launch table names, [(mode, multi, tile, b_kind, sup, (WM, WN, WK, TM, TN, NSLOT, NLA, NLB),
    (BM, BN), kernel symbol)], and blw_launch_ok's answer (0 / 1) to each of `lines` (the driver's header says how a line reads)"""
    global _driver
    if _driver is None:
        gxx = shutil.which("g++")
        assert gxx, "needs g++"
        d = tempfile.mkdtemp(prefix="blw_launch_table")
        atexit.register(shutil.rmtree, d, True)
        exe = os.path.join(d, "driver")
        subprocess.check_call([gxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I" + CSRC, os.path.join(ROOT, "tests", "blw_launch_table", "driver.cpp"), "-o", exe])
        _driver = exe
    out = subprocess.run([_driver], input="".join(l + "\n" for l in lines), capture_output=True, text=True, check=True, timeout=120).stdout.splitlines()
    inst = [l.split() for l in out if l.startswith("inst ")]
    ok = [int(l.split()[1]) for l in out if l.startswith("ok ")]
    assert len(inst) + len(ok) == len(out) and len(ok) == len(lines), out[-5:]
    return [tuple(int(x) for x in f[1:6]) + (tuple(int(x) for x in f[7:15]), (int(f[16]), int(f[17])), f[19]) for f in inst], ok
