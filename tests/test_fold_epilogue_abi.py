"""The epilogue fold's C-ABI entry points (xsmm_hip_set_fold_epilogue / xsmm_hip_fold_epilogue_stats) and their runtime.py wrappers;
no GPU needed: the switch and the counters are host state."""
import ctypes
import importlib

pkg = importlib.import_module("tpp-mlir_amd")


def test_fold_epilogue_exports_and_switch():
    rt = pkg.get_runtime()
    for name in ("xsmm_hip_set_fold_epilogue", "xsmm_hip_fold_epilogue_stats"):
        assert hasattr(rt.lib, name), name
    prev = rt.set_fold_epilogue(False)
    assert prev == 1  # default on (TPP_HIP_FOLD_EPILOGUE unset)
    assert rt.set_fold_epilogue(True) == 0
    assert rt.set_fold_epilogue(prev) == 1
    stats = rt.fold_epilogue_stats()
    assert len(stats) == 3 and all(isinstance(v, int) and v >= 0 for v in stats)
    out = (ctypes.c_int64 * 3)()
    rt.lib.xsmm_hip_fold_epilogue_stats(out)
    assert tuple(out) == stats
