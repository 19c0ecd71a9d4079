"""Worker of tests/test_trans_operands_gpu.py::test_strict_mode_folds_nothing: started with TPP_HIP_STRICT=1 and TPP_HIP_FOLD_TRANSPOSE=2 in
the environment (strict mode is chosen before the first invoke). Three (transpose, gemm) pairs whose gemm reads the temporary as its A
operand, through the tile queue; prints one JSON line: the fold mode the library read from the environment, the strict flag, the gemms
folded (none may be) and the largest deviation from the oracle."""
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import pyoracle as orc  # noqa: E402

pkg = importlib.import_module("tpp-mlir_amd")
rt = pkg.get_runtime()
import torch  # noqa: E402

F32, TRANSPOSE, BETA0, S, E = 1, 29, 4, 32, 512
rng = np.random.default_rng(45)
X, Bm = (rng.uniform(-1, 1, 4 * S * E).astype(np.float32) for _ in range(2))
ref, tmp = np.zeros(3 * S * 64, np.float32), np.zeros(S * S, np.float32)
for rep in range(3):
    orc.unary(TRANSPOSE, F32, S, S, E, S, 0, X, rep * 128, tmp, 0)
    orc.gemm(F32, S, 64, S, S, E, 64, BETA0, tmp, 0, Bm, rep * 64, ref, rep * S * 64)
mode = rt.lib.xsmm_hip_set_fold_transpose(2)
dX, dB, dT, dO = (torch.from_numpy(a.copy()).cuda() for a in (X, Bm, np.zeros(S * S, np.float32), np.zeros(3 * S * 64, np.float32)))
ht = rt.unary_dispatch(TRANSPOSE, F32, S, S, E, S, 0)
hg = rt.gemm_dispatch(F32, S, 64, S, S, E, 64, BETA0)
rt.set_async(True)
rt.set_tile_queue(1)
f0 = rt.fold_transpose_stats()
for rep in range(3):
    rt.unary(F32, ht, dX, rep * 128, dT, 0)
    rt.gemm(F32, hg, dT, 0, dB, rep * 64, dO, rep * S * 64)
rt.synchronize()
f1 = rt.fold_transpose_stats()
got = dO.cpu().numpy()
ok_tmp = bool(np.array_equal(dT.cpu().numpy(), tmp))
rt.set_tile_queue(0)
rt.set_async(False)
print(json.dumps({"mode_from_env": mode, "strict": rt.get_strict(), "folded": f1[0] - f0[0], "max_err": float(np.abs(got - ref).max()) if ok_tmp else 1e30,
                  "max_ref": float(np.abs(ref).max())}))
