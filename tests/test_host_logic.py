"""Host-side logic that needs no GPU: the MLP call decomposition, FLOP arithmetic and
the row-block partition used for multi-GPU sharding."""
import importlib
import json
import os

import pytest

pkg = importlib.import_module("tpp-mlir_amd")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_mlp_flops_match_mlir_gen_annotations():
    with open(os.path.join(GOLDEN, "flops.json")) as f:
        cases = json.load(f)["cases"]
    for c in cases:
        spec = pkg.MlpSpec(batch=c["batch"], layers=c["layers"], bias=c["bias"], relu=c["relu"])
        assert spec.flops() == c["flops"]
    # BASELINE config 4: 3 x (2*4096*1024*1024 + 2*4096*1024)
    assert pkg.MlpSpec().flops() == 25794969600


@pytest.mark.parametrize("batch,world", [(4096, 1), (4096, 2), (4096, 4), (4096, 8), (384, 2), (1000, 3), (128, 8)])
def test_row_partition_covers_batch_exactly(batch, world):
    parts = [pkg.row_partition(batch, world, r) for r in range(world)]
    row = 0
    for first, rows in parts:
        assert first == row and rows >= 0
        row += rows
    assert row == batch
    sizes = [p[1] for p in parts]
    assert max(sizes) - min(sizes) <= (128 if batch % 128 == 0 else 1)
    if batch % (128 * world) == 0:
        assert len(set(sizes)) == 1  # equal blocks -> a single all_gather_into_tensor


def test_layer_dispatch_tuple_matches_reference_fused_call():
    # the compiler emits (gemm_flags, unary_flags, unary_kind, binary_flags, binary_kind) = (.., 0, 5, 4, 1)
    # for bias + relu (test/Passes/pass-convert-mlp-to-parallel-tile.mlir:80)
    spec = pkg.MlpSpec(dtype=pkg.DataType.F32)
    args, br = pkg.layer_dispatch_args(spec, 512, 1024, 1024)
    assert (args["unary_flags"], args["unary_kind"], args["binary_flags"], args["binary_kind"]) == (0, 5, 4, 1)
    assert args["gemm_flags"] == 4 and br == 16 and args["stride_b"] == 64 * 1024
    spec = pkg.MlpSpec()
    args, _ = pkg.layer_dispatch_args(spec, 512, 1024, 1024)
    assert args["gemm_flags"] == 4 | 2048  # BETA_0 | wire value of vnni_b


def test_mlir_gen_seed_chain_matches_glibc():
    """oracle.pyoracle.glibc_rand_sequence restates glibc's rand() (mlir-gen seeds its dense constants from srand(seed) / rand(),
    MLIRGen.cpp:131-137, 810-819): pinned by the values glibc itself returns, and checked live against this host's libc"""
    import ctypes
    from oracle import pyoracle as orc
    assert orc.glibc_rand_sequence(123, 5) == [128959393, 1692901013, 436085873, 748533630, 776550279]
    assert orc.mlir_gen_seed_chain(123, 3) == [123, 128959393, 1692901013]
    libc = ctypes.CDLL(None)
    for seed in (1, 123, 2024, 0x7fffffff):
        libc.srand(seed)
        assert [libc.rand() for _ in range(40)] == orc.glibc_rand_sequence(seed, 40)



def test_bf16_loader_wave_kernels_do_not_spill():
    """every instance of brgemm_bf16_lw (single layers, chains, flat B) must fit the register file: a spilling instance still
    passes every parity test and runs 2-5x slower (seen twice while restructuring its MFMA loop) - so the build's own resource
    report is part of the suite"""
    import re
    import shutil
    import subprocess
    import tempfile
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("needs hipcc")
    src = os.path.join(ROOT, "tpp-mlir_amd", "csrc", "brgemm_bf16_lw.hip")
    with tempfile.TemporaryDirectory() as tmp:
        r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-c", src, "-o", os.path.join(tmp, "k.o"),
                            "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    names = re.findall(r"Function Name: (\S+)", r.stderr)
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)]
    assert len(names) == len(scratch) >= 18, (len(names), len(scratch))
    bad = [(n, s) for n, s in zip(names, scratch) if s != 0]
    assert not bad, "spilling kernels: %s" % bad


def test_shipped_library_has_no_measurement_switches():
    """the retired measurement and A/B switches - the chain kernel's timing bits and in-kernel stamps, and the environment
    variables that brought back an older kernel path - are gone: the library must not even contain their names"""
    import importlib
    build = importlib.import_module("tpp-mlir_amd.build")
    blob = open(build.build(), "rb").read()
    for name in (b"TPP_HIP_CHAIN_DBG", b"TPP_HIP_CHAIN_STAMPS",
                 b"TPP_HIP_F32_LW16", b"TPP_HIP_BF16_LONG_K", b"TPP_HIP_BF16_LW32", b"TPP_HIP_GROUPED_K32_PAIRS",
                 b"TPP_HIP_BF16_LW_GROUPED", b"TPP_HIP_BF16_LW_RAGGED", b"TPP_HIP_BF16_LW_T4_VNNI4", b"TPP_HIP_BF16_QUADS",
                 b"TPP_HIP_BF16_LW\0", b"TPP_HIP_BF16_LW_PICK", b"TPP_HIP_BF16_LW_XM", b"TPP_HIP_BLW_SUP", b"TPP_HIP_BLW_T3",
                 b"TPP_HIP_F32_LW_XM", b"TPP_HIP_F32_LW_C3_LOADERS", b"TPP_HIP_TRANSPOSE_TILE", b"TPP_HIP_PACK_PIECE",
                 b"TPP_HIP_PACK_POLICY", b"TPP_HIP_PEER_FINEGRAINED", b"TPP_HIP_QUEUE_SOLO", b"TPP_HIP_GRID_MERGE"):
        assert name not in blob, name


def _run_bench(argv, env_extra, drop=("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")):
    import subprocess
    import sys
    env = {k: v for k, v in os.environ.items() if k not in drop}
    env.update(env_extra)
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + argv, capture_output=True, text=True, env=env, timeout=600, cwd=ROOT)


def test_bench_refuses_a_world_size_that_differs_from_gpus():
    """never an N = 1 line under an N > 1 command - a launcher-set WORLD_SIZE that differs from --gpus is an
    error for world == 1 too (checked before anything touches a GPU)"""
    r = _run_bench(["--gpus", "8", "--steps", "2", "--warmup", "1"], {"WORLD_SIZE": "1", "RANK": "0", "LOCAL_RANK": "0"})
    assert r.returncode != 0 and "--gpus 8 but WORLD_SIZE=1" in r.stderr and "{" not in r.stdout
    r = _run_bench(["--gpus", "1", "--steps", "2", "--warmup", "1"], {"WORLD_SIZE": "2", "RANK": "0", "LOCAL_RANK": "0"})
    assert r.returncode != 0 and "--gpus 1 but WORLD_SIZE=2" in r.stderr and "{" not in r.stdout


def test_bench_gpus_n_without_world_size_launches_n_ranks():
    """`python bench.py --gpus 2` with no launcher starts two ranks itself (here, without a GPU, each rank stops at 'needs an
    MI355X' - what matters is that TWO ranks with WORLD_SIZE=2 were started, no JSON line was printed and the exit code is not 0)"""
    r = _run_bench(["--gpus", "2", "--steps", "2", "--warmup", "1"], {})
    assert "launching 2 ranks" in r.stderr and "torch.distributed.run" in r.stderr
    import torch
    if not torch.cuda.is_available():
        assert r.returncode != 0 and r.stderr.count("needs an MI355X") >= 2, r.stderr[-3000:]
        assert not [l for l in r.stdout.splitlines() if l.startswith("{")]


def test_bench_refuses_fewer_than_one_timed_step():
    """ms_per_step is the wall time of the timed steps / --steps: zero steps is an error, before anything touches a GPU"""
    r = _run_bench(["--gpus", "1", "--steps", "0", "--warmup", "1"], {})
    assert r.returncode != 0 and "--steps must be >= 1" in r.stderr and "{" not in r.stdout


def test_bench_dump_outputs_writes_float32_npy_within_the_limit(tmp_path):
    """--dump-outputs: every array as DIR/<name>.npy in float32 (bf16 / f32 values exactly), 64 MB in all at most"""
    import importlib.util
    import numpy as np
    spec = importlib.util.spec_from_file_location("bench_mod3", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    rng = np.random.default_rng(5)
    arrays = {"c2_C": rng.standard_normal((64, 32)).astype(np.float32), "mlp_out": rng.standard_normal((16, 8))}
    shapes = bench.dump_outputs(str(tmp_path / "out"), arrays)
    assert shapes == {"c2_C": [64, 32], "mlp_out": [16, 8]}
    for name, a in arrays.items():
        got = np.load(str(tmp_path / "out" / (name + ".npy")))
        assert got.dtype == np.float32 and np.array_equal(got, a.astype(np.float32))
    big = {"x": np.zeros(bench.DUMP_LIMIT_BYTES // 4 + 1, np.float32)}
    with pytest.raises(SystemExit):
        bench.dump_outputs(str(tmp_path / "big"), big)
    assert not os.path.exists(str(tmp_path / "big"))


def test_bench_final_line_is_compact_and_keeps_every_baseline_config():
    """the driver keeps an 8 KB tail of bench.py's stdout; round 5's ONE line had grown to 16 KB and the
    driver-written record lost the C4 step. The final line is now a pure function of the full line (bench.compact_line): under
    4 KB, with the contract keys, roofline + cpu_baseline objects and one figure per BASELINE config. Checked here on committed
    full lines of earlier rounds (N = 1) and on the N = 2 rig line."""
    import importlib.util
    import json
    spec = importlib.util.spec_from_file_location("bench_mod2", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    for name in ("r04_bench.json", "r05_bench.json", "r05_bench_steps20.json", "r05_bench_gpus2_rig.json"):
        full = json.loads([l for l in open(os.path.join(ROOT, "profiles", name)).read().splitlines() if l.startswith("{")][-1])
        out = bench.compact_line(full)
        text = json.dumps(out)
        assert len(text) < 4096, (name, len(text))
        for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data"):
            assert out[k] == full[k], (name, k)
        assert out["config"]["workload"] == full["config"]["workload"]
        roof = out["roofline"]
        for k in ("bound", "achieved", "peak", "unit", "frac"):
            assert roof[k] == full["roofline"][k], (name, k)
        assert "traffic" in roof
        c4 = roof["configs"]["C4"]
        assert c4["ms_per_step"] == full["mlp"]["ms_per_step"] and c4["frac"] == full["mlp"]["frac_of_bf16_mfma_peak"]
        if full["n_gpus"] == 1:
            assert roof["configs"]["C3"]["us"] > 0 and roof["configs"]["C5"]["us"] > 0
            cb = out["cpu_baseline"]
            assert cb["value"] == full["cpu_baseline"]["value"] and cb["cores"] == full["cpu_baseline"]["cores"] and cb["kind"] == "port"
            assert len(cb["sample"]) <= 260
        else:
            assert c4["gathered_bit_identical"] is True and out["process_group"]["world_size"] == full["n_gpus"]
            assert out["c2_weak"]["value"] == full["c2_weak"]["value"]


def test_refbench_restates_the_reference_benchmark_configs():
    """tools/refbench.py's shape table = the IR-GEN rows of benchmarks/config/matmul/*.json and fc/*.json (harvested into
    tests/golden/benchmark_configs.json by tests/golden/harvest_benchmarks.py): same (batch, out, in) shapes, same --tiles, the fc
    rows with --bias --relu, --kernel=args, f32 / bf16 vnni 2 / bf16 vnni 4 each; base.json's tiled gemm / mlp rows 256 x 1024 x 3"""
    import importlib.util
    spec = importlib.util.spec_from_file_location("refbench", os.path.join(ROOT, "tools", "refbench.py"))
    rb = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(rb)
    with open(os.path.join(GOLDEN, "benchmark_configs.json")) as f:
        cfg = json.load(f)
    for fam in ("matmul", "fc"):
        want = {(r["batch"], r["layers"][1], r["layers"][0], tuple(r["tiles"])) for r in cfg[fam]}
        assert want == set(rb.SHAPES), (fam, want ^ set(rb.SHAPES))
        assert all(r["kernel"] == "args" and r["bias"] == (fam == "fc") and r["relu"] == (fam == "fc") for r in cfg[fam])
        assert {(r["float_type"], r["vnni"]) for r in cfg[fam]} == {("f32", 0), ("bf16", 2), ("bf16", 4)}
    tiled = [r for r in cfg["base"] if r["tiles"]]
    assert tiled and all(r["batch"] == 256 and r["layers"] == [1024] * 4 and r["tiles"] == [32, 32, 32] and r["kernel"] == "const" for r in tiled)
    got = rb.cases("")
    assert len([c for c in got if c["family"] != "mlir"]) == (17 + 17) * 3 * 2 + 2 * 3 * 2
    # the hand-written files of base/mha.json and pack.json (benchmarks/mlir/*.mlir) as call scripts: every file the tree holds, its own
    # BENCH_TOTAL_FLOPS, and per tile the dispatches the reference's conversion test pins (linalg-to-gemm.mlir; zero fills folded into BETA_0)
    files = {r["file"]: r for r in cfg["mlir"]["files"] if r["in_tree"]}
    scripts = [c for c in got if c["family"] == "mlir"]
    assert {c["cite"] for c in scripts} == set(files) and len(scripts) == 6
    assert all(c["flops"] == files[c["cite"]]["bench_total_flops"] for c in scripts)
    fn = {"mha_projection": "mha_projection", "mha_qk": "mha_query_times_key", "mha_sv": "mha_out_softmax_times_value"}
    for script, calls in rb.SCRIPT_CALLS.items():
        pinned = [(("%s %s" % (c["op"], c["kind"])) if c["kind"] else c["op"], c["dims"]) for c in cfg["mlir"]["lowered_calls"][fn[script]] if c["kind"] != "zero"]
        assert pinned == [(op, dims) for op, dims in calls], (script, pinned)
        assert all(c["flags"] == "none" for c in cfg["mlir"]["lowered_calls"][fn[script]] if c["kind"] != "zero")
    # ... and tools/tpp_replay.cpp issues exactly those tuples (S = 32, D = 64, E = 512 in its --script mode)
    src = open(os.path.join(ROOT, "tools", "tpp_replay.cpp")).read()
    for needle in ("xsmm_gemm_dispatch(1, S, D, E, E, E, E, XSMM_GEMM_FLAG_BETA_0)", "xsmm_unary_dispatch(XSMM_UNARY_TRANSPOSE, 1, S, D, E, S, 0)",
                   "xsmm_gemm_dispatch(1, S, S, D, E, S, S, XSMM_GEMM_FLAG_BETA_0)", "xsmm_gemm_dispatch(1, S, D, S, S, E, E, XSMM_GEMM_FLAG_BETA_0)",
                   "Bt = 64, S = 32, H = 8, D = 64, E = H * D"):
        assert needle in src, needle
    # ... and bench.py's cpu_baseline leg (the CPU column of the table) runs the same (M, N, K) list
    spec_b = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    bm = importlib.util.module_from_spec(spec_b)
    spec_b.loader.exec_module(bm)
    assert bm.REFBENCH_SHAPES == [(M, N, K) for (M, N, K, _) in rb.SHAPES]
    assert {c["kernel"] for c in got if c["family"] == "base"} == {"const"} and {c["kernel"] for c in got if c["family"] in ("matmul", "fc")} == {"args"}
