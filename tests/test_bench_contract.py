"""The driver's contract for bench.py, checked on the committed lines of the last GPU runs (profiles/r06_*.json; config 5: r04_*, r05_config5_* and
r06_config5_*): the one JSON line carries BASELINE.json's metric with every field the contract names, a roofline object for the dominant kernel and
a CPU baseline (a --full run); and the command line still parses the driver's flags.  (No GPU: the line is a committed measurement.  One
-m gpu test runs a plain line and checks the outputs it dumps.)"""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _line(name):
    with open(os.path.join(ROOT, "profiles", name)) as fh:
        return json.loads(fh.read().strip().splitlines()[-1])


def test_default_line_has_every_contract_field():
    l = _line("r06_bench_default.json")
    assert l["metric"] == "segments/sec" and l["unit"] == "segments/s" and l["higher_is_better"] is True
    assert l["n_gpus"] == 1 and l["steps"] == 60 and l["warmup"] == 2 and l["scaling"] == "weak" and l["data"] == "synthetic"
    assert l["vs_baseline"] is None and l["dtype"] == "u32"                      # BASELINE.md publishes no number for this metric
    assert abs(l["value"] - 1e3 / l["ms_per_step"]) / l["value"] < 1e-6 and "workload" in l["config"] and "model" not in l["config"]
    assert l["steps"] * l["ms_per_step"] >= 1390.0                               # the timed region is about 1.4 s
    assert l["command_wall_s"] - l["build_s"] <= 75.0                            # the default command: about a minute once built
    r = l["roofline"]
    assert r["bound"] in ("hbm", "mfma") and r["unit"] in ("GB/s", "TFLOP/s") and r["peak"] == 8000.0
    assert abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-9 and r["kernel"] == "hash_rows"
    assert 0.99 < r["traffic"] / r["alg_bytes_per_launch"] < 1.01 and "measured in this run" in r["traffic_source"]
    # the roofline that BINDS the dominant kernel, measured live: VALU wave-instructions per SIMD-cycle against the half-rate class's 0.25
    v = r["valu"]
    assert abs(v["issue_frac"] - v["wave_instr"] / v["simd_cycles"]) < 1e-9 and 0.2 < v["issue_frac"] <= 0.25 and v["half_rate_share"] == 0.85
    assert "SQ_INSTS_VALU" in v["source"] and 0.15 < r["seal_valu_issue_frac"] <= 0.26 and r["seal_valu_wave_instr"] > 1e10
    # ... and against the ALGORITHMIC VALU work of a Poseidon2 permutation (22.3 k SIMD-cycles per 64 permutations): ~0.83 at the sustained clock
    assert v["algorithmic_floor_cycles"] == 1356 * 12 + 6000 and abs(v["frac_of_algorithmic_floor"] - v["algorithmic_floor_cycles"] / v["cycles_per_wave_permutation"]) < 1e-9
    assert 0.75 < v["frac_of_algorithmic_floor"] < 0.95 and 0.6 < v["frac_of_algorithmic_floor_at_2p4GHz"] < v["frac_of_algorithmic_floor"]
    assert abs(l["config"]["dominant_valu_algorithmic_frac"] - v["frac_of_algorithmic_floor"]) < 1e-3
    # the CPU baseline: one seal alone AND every core busy, the CPU named (round 6)
    c = l["cpu_baseline"]
    assert c["kind"] in ("reference", "port") and c["cores"] >= 1 and c["value"] > 0 and c["unit"] == "segments/s" and c["sample"]
    assert "EPYC" in c["cpu_model"] and c["cpu_model"] in c["sample"] and c["cores_available"] == 256
    assert c["single_seal"]["value"] > 0 and c["full_host"]["cores"] == 256 and c["full_host"]["processes"] >= 4 and c["full_host"]["value"] > 0
    assert c["value"] == max(c["single_seal"]["value"], c["full_host"]["value"])
    # the line certifies its own work, and folds a block to one receipt
    assert l["timed_seals_verified"] == 60 and l["seal_matches_golden"] is True
    b = l["block"]
    assert b["verified_after_clock"] == b["segments"] == 64
    assert b["recursive"]["root_verified_against_leaf_claims"] is True and b["recursive"]["proofs"] == 49        # 32 lift2 + 17 join3 / joins (binary: 63)
    assert "resident" in b["code_group"] and b["recompute_code_group"]["segments_per_s"] > 0
    assert l["block_wall_clock_s"] == b["wall_clock_s"] and l["block_segments_per_s"] == b["segments_per_s"]
    # row f1: the host-preflight pipeline, with the Amdahl term and the PCIe bytes in the line
    p = b["host_preflight_pipeline"]
    assert p["segments_per_s"] >= 41.0 and p["verified_after_clock"] == 64 and p["host_preflight_cpu_ms_per_segment"] > 1.0
    assert p["pcie_bytes_per_segment"] < 0.02 * p["full_trace_bytes_per_segment"]
    assert abs(p["host_cores_needed"] - p["segments_per_s"] * p["host_preflight_cpu_ms_per_segment"] / 1e3) < 1e-6 and p["reps"] == 2 and p["min"] <= p["max"]
    # what a record that keeps only the contract's keys (and drops nested objects) still holds: SCALAR keys of `config`, none longer
    # than 32 characters (round 5's driver record cut one at 40)
    cfg = l["config"]
    assert "numa_node" in cfg["host_placement_rank0"] and cfg["value_recomputes_code_group"] is True and "re-committed per segment" in cfg["workload"]
    assert max(len(k) for k in cfg) <= 32
    for key in ("syn_heavy_segments_per_s", "syn_heavy_min_segments_per_s", "syn_heavy_max_segments_per_s", "syn_heavy_ms_per_step", "block_segments_per_s",
                "resident_code_segments_per_s", "preflight_segments_per_s", "preflight_host_cores_needed", "block_recompute_segments_per_s",
                "dominant_kernel_valu_issue_frac", "seal_valu_issue_frac", "seal_hbm_frac", "block_fold_to_one_receipt_s",
                "syn_heavy_eval_instr_per_point", "syn_heavy_eval_valu_issue_frac", "syn_heavy_seal_valu_issue_frac"):
        assert isinstance(cfg[key], (int, float)) and cfg[key] > 0, key
    assert "also_measured" not in cfg and abs(cfg["syn_heavy_segments_per_s"] - l["syn_heavy"]["segments_per_s"]) < 1e-2
    # who ran it: the device list, the launcher, the RCCL probe, the parity pins (none dropped yet)
    assert cfg["launcher"] == "ranks" and len(cfg["devices"]) == 1 and cfg["devices_distinct"] is True and cfg["devices"][0]["pci_bus_id"] and cfg["devices"][0]["uuid"]
    assert cfg["rccl_probe"] is None and cfg["parity_pins"] is None


def test_secondary_legs_are_repeated_and_syn_heavy_is_first_class():
    """round-5 verdict, item 1: every secondary figure is timed twice after a real warm-up and carries {value, min, max}; SYN-HEAVY is an
    object beside `value` with its own VALU roofline; five runs of the driver's command on one lease agree within a few per cent"""
    l = _line("r06_bench_default.json")
    h = l["syn_heavy"]
    assert h["reps"] == 2 and h["steps"] == 18 and h["min"] <= h["segments_per_s"] <= h["max"] and h["value"] == h["segments_per_s"] and h["unit"] == "segments/s"
    assert h["spread_pct"] < 8.0 and "unstable" not in h and abs(h["ms_per_step"] - 1e3 / h["segments_per_s"]) < 0.05
    hv = h["roofline"]["valu"]
    assert h["roofline"]["kernel"] == "eval_check" and 74000 < hv["instr_per_point"] < 82000 and 0.2 < hv["issue_frac"] < 0.3      # 105.6 k before round 6; 83.9 k after LINFORM alone
    assert h["segments_per_s"] >= 30.0 and h["kernels_ms_per_seal_unshared"]["eval_check"] < 10.0                                  # 28.4 / 11.9 ms before
    rc = l["code_group_resident"]
    assert rc["reps"] == 2 and rc["min"] <= rc["segments_per_s"] <= rc["max"] and rc["seals_identical_to_recomputing_prover"] is True
    s = json.load(open(os.path.join(ROOT, "profiles", "r06_repro_summary.json")))
    assert len(s["value"]["runs"]) == 5 and s["value"]["spread_pct"] <= 5.0 and s["syn_heavy"]["spread_pct"] <= 5.0 and s["unstable_legs"] == []
    assert s["resident_code"]["spread_pct"] <= 5.0 and s["block"]["spread_pct"] <= 5.0 and s["preflight"]["spread_pct"] <= 5.0
    d = _line("r06_bench_driver_cmd.json")
    assert abs(d["syn_heavy"]["segments_per_s"] - s["syn_heavy"]["mean"]) / s["syn_heavy"]["mean"] <= 0.05


def test_the_drivers_command_fits_in_a_minute():
    l = _line("r06_bench_driver_cmd.json")                                       # python bench.py --gpus 1 --steps 20 --warmup 5
    assert l["steps"] == 20 and l["warmup"] == 5 and l["command_wall_s"] <= 70.0 and l["timed_seals_verified"] == 20
    assert l["roofline"]["valu"]["issue_frac"] > 0.2 and l["cpu_baseline"]["value"] > 0


def test_eight_rank_line_is_contract_complete():
    """The driver's multi-GPU command, dry-run as 8 ranks on ONE GPU (--allow-shared-gpu / ZKH_SHARE_GPUS=1): a SCALE line shaped like this must not
    come back unmeasured — roofline with a non-zero fraction, measured traffic and VALU issue, a CPU baseline, the strong-scaling leg — and it
    says WHICH devices its ranks held (round 6): eight entries, here all the same GPU, `devices_distinct: false`."""
    l = _line("r06_8rank_one_gpu.json")
    assert l["n_gpus"] == 8 and l["scaling"] == "weak" and l["timed_seals_verified"] == 8 * l["steps"] and l["seal_matches_golden"] is True
    assert "failed_ranks" not in l
    cfg = l["config"]
    assert [d["rank"] for d in cfg["devices"]] == list(range(8)) and cfg["devices_distinct"] is False and cfg["distinct_devices"] == 1
    assert all(d["pci_bus_id"] == cfg["devices"][0]["pci_bus_id"] and d["uuid"] for d in cfg["devices"]) and cfg["rccl_probe"] is None
    r = l["roofline"]
    assert r["frac"] > 0 and r["alg_bytes_per_launch"] > 0 and r["traffic"] is not None and r["traffic"] > 0 and r["kernel"] == "hash_rows"
    assert abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-9 and r["valu"]["issue_frac"] > 0.2
    c = l["cpu_baseline"]
    assert c["value"] > 0 and c["cores"] >= 1 and c["kind"] == "port" and c["sample"]
    b = l["block"]
    assert b["segments"] == 256 == b["verified_after_clock"] and l["block_wall_clock_s"] > 0 and l["block_segments_per_s"] > 0
    assert b["host_preflight_pipeline"]["verified_after_clock"] == 256
    t = _line("r06_torchrun2_one_gpu.json")                                      # python -m torch.distributed.run ... bench.py --gpus 2
    assert t["n_gpus"] == 2 and t["timed_seals_verified"] == 16 and t["block"]["verified_after_clock"] == 256 and len(t["config"]["devices"]) == 2


def test_the_session_launcher_and_the_rccl_probe_on_one_gpu():
    """--launcher session: the N-GPU headline as ONE process (zkh_session_create with N devices x K lanes); and what the RCCL health probe
    says where it can run: world 1 "ok"; forced on two ranks sharing one GPU RCCL refuses and the line is still printed"""
    s8, s1 = _line("r06_session_8dev_one_gpu.json"), _line("r06_session_1gpu.json")
    for l, n in ((s8, 8), (s1, 1)):
        cfg = l["config"]
        assert l["n_gpus"] == n and cfg["launcher"] == "session" and len(cfg["devices"]) == n and cfg["witgen_in_clock"] is True
        assert l["timed_seals_verified"] == n * l["steps"] and l["seal_matches_golden"] is True and l["roofline"]["frac"] > 0 and l["cpu_baseline"]["value"] > 0
        assert "INSIDE the clock" in cfg["workload"] and max(len(k) for k in cfg) <= 32
    assert s8["config"]["devices_distinct"] is False and s1["config"]["devices_distinct"] is True
    assert s8["value"] > 41.0 and s1["value"] > 41.0                              # one process, no launcher: the GPU's rate
    p = json.loads(open(os.path.join(ROOT, "profiles", "r06_rccl_probe_world1.json")).read().splitlines()[0])     # (RCCL prints its version banner after it)
    assert p["rccl_probe"] == "ok" and p["rccl_world"] == 1 and p["hung"] is False
    f = _line("r06_2rank_forced_rccl_one_gpu.json")
    assert f["n_gpus"] == 2 and f["config"]["rccl_probe"].startswith("unavailable (") and f["config"]["rccl_world"] is None and f["value"] > 0


def test_a_faulting_rank_on_the_gpu_leaves_the_survivors_line():
    """4 ranks on one GPU, rank 2 raises inside the headline leg (ZKH_BENCH_FAULT_RANK=2): the line is there within seconds, it
    counts the three survivors, says who failed, and nothing else is attempted on the broken group (tests/test_bench_faults.py
    runs the same paths on CPU through --config dev)."""
    l = _line("r05_4rank_fault_one_gpu.json")
    assert l["n_gpus"] == 4 and l["failed_ranks"] == [2] and l["failed_in"] == "headline" and l["ranks_reporting"] == 3 and l["value"] > 0
    assert "skipped" in l["block"] and "cpu_baseline" not in l and l["roofline"]["traffic"] is None


def test_config5_line_is_the_streamed_in_circuit_fold():
    l = _line("r04_bench_succinct_streamed.json")
    r = l["recursion"]
    assert l["steps"] == 1024 and l["succinct_root_follows_from_leaf_claims"] is True and "recursion" in l["config"]["join_circuit"]
    assert r["fused_lift2"] == 512 and r["joins"] == 511 and r["proofs"] == 1023 and l["verified_after_clock"] >= 1025
    assert r["streamed_fold"] is True and r["fold_tail_s"] < 0.5 and "native" in r["executor"]
    two = _line("r04_bench_succinct_phased.json")
    assert two["recursion"]["streamed_fold"] is False and two["recursion"]["fold_tail_s"] > 3.0
    assert l["block_wall_clock_s"] < two["block_wall_clock_s"] < 27.8                   # round 3: 27.8 s
    host = _line("r04_prove_session_recursion_1024_streamed.json")                       # the g++ host, no Python in the process
    assert host["wall_s"] <= 26.5 and host["streamed_fold"] is True and host["verified"] is True and host["joins"] == 511      # 25.7-26.3 s over boxes
    # ... and with three children per proof above the bottom level (conditional-swap blocks made the room): 768 proofs, not 1 023
    j3, no3 = _line("r04_prove_session_recursion_1024_join3.json"), _line("r04_prove_session_recursion_1024_no_join3.json")
    assert j3["lifts"] == no3["lifts"] == 512 and j3["joins"] == 256 and no3["joins"] == 511 and j3["verified"] is no3["verified"] is True
    assert j3["wall_s"] < no3["wall_s"] and j3["wall_s"] <= 25.5 and j3["fold_busy_lane_s"] < 0.85 * no3["fold_busy_lane_s"]
    ph = _line("r04_prove_session_recursion_1024_join3_two_phase.json")                  # the fold on its own: round 3's 4.2 s -> 3.1 s
    assert ph["streamed_fold"] is False and ph["lift_s"] + ph["join_tree_s"] <= 3.3 and ph["verified"] is True
    b3 = _line("r04_bench_succinct_join3.json")
    assert b3["recursion"]["proofs"] == 768 and b3["succinct_root_follows_from_leaf_claims"] is True and b3["block_wall_clock_s"] < l["block_wall_clock_s"]


def test_config5_on_the_final_tree_of_round5_incl_assumption_receipts():
    """profiles/r05_config5_*.json: the same 1024-segment block through the round-5 executor (csrc/scheduler.h), programs built by the
    library; and the same session ASSUMING 8 keccak receipts - 8 more lifts, 7 unions, one resolve - for 0.1 s more"""
    host = _line("r05_config5_prove_session_1024.json")
    assert host["segments"] == 1024 and host["lifts"] == 512 and host["joins"] == 256 and host["verified"] is True and host["programs_built_by_library"] is True
    assert host["wall_s"] <= 26.5 and host["fold_tail_s"] < 0.5 and host["resolved"] is False
    k8 = _line("r05_config5_prove_session_1024_keccak8.json")
    assert k8["assumption_receipts"] == 8 and k8["resolved"] is True and k8["verified"] is True
    assert k8["lifts"] == 512 + 8 and k8["joins"] == 256 + 7 + 1 and k8["wall_s"] < host["wall_s"] + 0.5 and k8["root_out"] != host["root_out"]
    assert k8["root_out"][64:] != host["root_out"][64:]                                   # another program set: another allowed-programs root
    b = _line("r05_config5_bench_succinct.json")
    assert b["steps"] == 1024 and b["recursion"]["proofs"] == 768 and b["succinct_root_follows_from_leaf_claims"] is True and b["verified_after_clock"] >= 1025
    assert b["block_wall_clock_s"] < 27.8 and b["recursion"]["fold_tail_s"] < 0.5
    # ... and on round 6's tree (the NTT / Merkle experiment variants removed from the library, the generator's analyses on the effective roots)
    b6 = _line("r06_config5_bench_succinct_streamed.json")
    assert b6["steps"] == 1024 and b6["recursion"]["proofs"] == 768 and b6["succinct_root_follows_from_leaf_claims"] is True and b6["verified_after_clock"] >= 1025
    assert b6["block_wall_clock_s"] < 26.5 and b6["recursion"]["fold_tail_s"] < 0.5
    h6 = _line("r06_config5_prove_session_1024_streamed.json")
    assert h6["segments"] == 1024 and h6["lifts"] == 512 and h6["joins"] == 256 and h6["verified"] is True and h6["wall_s"] <= 26.0


def test_bench_accepts_the_drivers_flags():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0
    for flag in ("--gpus", "--steps", "--warmup", "--config", "--join-circuit", "--fold-inflight", "--no-fused-lift", "--fold", "--executor",
                 "--recompute-code", "--no-preflight-leg", "--no-join3", "--witness", "--cpu-full-host", "--with-p2-join", "--full", "--dump-outputs"):
        assert flag in out.stdout, flag


def test_a_plain_run_is_the_headline_and_full_is_opt_in():
    """`bench.py --gpus 1 --steps K --warmup W` times the K steps and prints the line; certification, the secondary legs, the roofline and
    the CPU baseline run with --full only.  --dump-outputs belongs to the segment config's ranks launcher."""
    bench = _load_bench()
    a = bench.parse_args(["--gpus", "1", "--steps", "7", "--warmup", "3"])
    assert bench.lean(a) and not a.full and a.dump_outputs is None and a.steps == 7 and a.warmup == 3
    assert not bench.lean(bench.parse_args(["--full"])) and bench.parse_args(["--dump-outputs", "d"]).dump_outputs == "d"
    assert not bench.lean(bench.parse_args(["--config", "block"])) and not bench.lean(bench.parse_args(["--launcher", "session"]))
    for bad in (["--config", "block", "--dump-outputs", "d"], ["--launcher", "session", "--dump-outputs", "d"]):
        out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *bad], capture_output=True, text=True, timeout=120)
        assert out.returncode == 2 and "--dump-outputs" in out.stderr and not out.stdout


def test_dump_outputs_writes_exact_float64(tmp_path):
    import numpy as np
    from benchlib.common import DUMP_LIMIT_BYTES, dump_outputs
    seal = np.array([0, 1, 2013265920, 0xFFFFFFFF], dtype=np.uint32)
    half = np.linspace(-1, 1, 5, dtype=np.float32)
    paths = dump_outputs(str(tmp_path / "out"), {"seal": seal, "half": half})
    assert sorted(os.path.basename(p) for p in paths) == ["half.npy", "seal.npy"]
    s = np.load(tmp_path / "out" / "seal.npy")
    h = np.load(tmp_path / "out" / "half.npy")
    assert s.dtype == np.float64 and np.array_equal(s.astype(np.uint64), seal.astype(np.uint64))
    assert h.dtype == np.float32 and np.array_equal(h, half)
    with pytest.raises(ValueError, match="bytes"):
        dump_outputs(str(tmp_path / "big"), {"x": np.zeros(DUMP_LIMIT_BYTES // 8 + 1, dtype=np.uint32)})
    with pytest.raises(ValueError, match="exactly"):
        dump_outputs(str(tmp_path / "wide"), {"x": np.array([1 << 60], dtype=np.uint64)})
    assert not (tmp_path / "big").exists() and not (tmp_path / "wide").exists()


@pytest.mark.gpu
def test_a_plain_run_dumps_the_last_steps_seal(hal, tmp_path):
    """A plain run on the GPU: the line says what it measured and nothing else ran; --dump-outputs holds the receipt of the last timed step.
    Step k of K seals ring slot (W + k) mod 2, so K = 4 and K = 5 end on different segments: each dump must be the seal of ITS slot's segment
    (not the other's), and the host verifier must accept it."""
    import numpy as np
    from benchlib.common import BASE_SEED, BENCH_NOISE
    from zeth_amd.circuits import syn_air
    from zeth_amd.prover import Segment, SegmentProver, SegmentReceipt
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "ZKH_SHARE_GPUS")}
    warmup, inflight, po2 = 1, 2, 16
    desc = syn_air.syn_a()
    prover = SegmentProver(hal, desc)
    want = [prover.prove_segment(Segment(index=k, po2=po2, seed=BASE_SEED + k, noise_seed=BENCH_NOISE)) for k in range(2)]
    assert not np.array_equal(want[0].seal, want[1].seal)
    for steps in (4, 5):
        out_dir = tmp_path / f"k{steps}"
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup), "--po2", str(po2),
                            "--inflight", str(inflight), "--dump-outputs", str(out_dir)], env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        l = json.loads(r.stdout.strip().splitlines()[-1])
        assert l["metric"] == "segments/sec" and l["unit"] == "segments/s" and l["higher_is_better"] is True and l["dtype"] == "u32"
        assert l["steps"] == steps and l["warmup"] == warmup and abs(l["value"] - 1e3 / l["ms_per_step"]) / l["value"] < 1e-6
        assert l["config"]["full_run"] is False and l["config"]["build_current"] is True
        for key in ("certify", "block", "syn_heavy", "code_group_resident", "roofline", "cpu_baseline", "timed_seals_verified"):
            assert key not in l, key
        slot = (warmup + steps - 1) % 2
        seal, out = np.load(out_dir / "seal.npy"), np.load(out_dir / "output.npy")
        assert seal.dtype == np.float64 and out.dtype == np.float64
        seal, out = seal.astype(np.uint32), out.astype(np.uint32)
        assert np.array_equal(seal, want[slot].seal) and np.array_equal(out, want[slot].output), steps
        assert not np.array_equal(seal, want[1 - slot].seal), steps
        SegmentReceipt(seal=seal, index=slot, po2=po2, output=out).verify(desc, prover.control_root(po2))


def _load_bench():
    import importlib.util
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_roofline_is_taken_per_op_and_never_from_a_byteless_sub_kernel_bracket():
    """Round-3 verdict, weak 8: on a shared GPU a sub-kernel bracket of a multi-pass op (whose §8d bytes are charged to another
    pass of the same op) out-timed everything and the line said frac 0.0 / alg_bytes 0.0.  The dominant entry is now an OP:
    passes summed, bytes summed, invocations = calls of the byte-carrying passes."""
    bench = _load_bench()
    recs = [{"name": "hash_rows", "calls": 7, "total_ms": 14.0, "alg_bytes": 7 * 740e6},
            {"name": "batch_expand_into_evaluate_ntt:k_ntt_high10", "calls": 5, "total_ms": 30.0, "alg_bytes": 0.0},      # queued behind other ranks
            {"name": "batch_expand_into_evaluate_ntt:k_ntt_low12", "calls": 6, "total_ms": 2.0, "alg_bytes": 6 * 700e6},
            {"name": "batch_expand_into_evaluate_ntt:k_ntt_pass", "calls": 3, "total_ms": 0.1, "alg_bytes": 3 * 1e5},
            {"name": "syn_data", "calls": 1, "total_ms": 50.0, "alg_bytes": 0.0}]                                          # a bracket with no §8d bytes at all
    ops = bench.by_op(recs)
    ntt = ops["batch_expand_into_evaluate_ntt"]
    assert ntt["calls"] == 9 and ntt["launches"] == 14 and abs(ntt["total_ms"] - 32.1) < 1e-9 and ntt["alg_bytes"] > 4e9

    class A:
        no_live_traffic, circuit, po2, steps = True, "syn_a", 20, 1
    line = {}
    bench.add_roofline(line, recs, recs, A, 3, (32, 16, 208), 1 << 20)
    r = line["roofline"]
    assert r["kernel"] == "batch_expand_into_evaluate_ntt" and r["frac"] > 0 and r["alg_bytes_per_launch"] > 0 and r["achieved"] > 0
    assert abs(r["avg_launch_ms"] - 32.1 / 9) < 1e-9
    # with hash_rows dominant the committed PMC file supplies the traffic when no live measurement is possible
    recs[1]["total_ms"] = 3.0
    recs[4]["total_ms"] = 0.5
    line = {}
    bench.add_roofline(line, recs, recs, A, 3, (32, 16, 208), 1 << 20)
    r = line["roofline"]
    assert r["kernel"] == "hash_rows" and r["traffic"] and r["traffic"] > 0 and abs(r["alg_bytes_per_launch"] - 740e6) < 1
    assert [o["op"] for o in line["ops"]][:2] == ["hash_rows", "batch_expand_into_evaluate_ntt"]


def test_host_placement_helpers_parse_sysfs(tmp_path):
    """csrc/topology.hip without a GPU: cpulist parsing, PCI function -> NUMA node -> CPUs under a fake sysfs tree."""
    from zeth_amd import hal
    assert hal.parse_cpulist("0-3,8,10-11\n") == [0, 1, 2, 3, 8, 10, 11]
    assert hal.parse_cpulist("5") == [5] and hal.parse_cpulist("") == []
    for bad in ("abc", "3-1", "1-", "0-3;5"):
        try:
            hal.parse_cpulist(bad)
            raise AssertionError(bad)
        except hal.HalError:
            pass
    dev = tmp_path / "bus" / "pci" / "devices" / "0000:c1:00.0"
    dev.mkdir(parents=True)
    (dev / "numa_node").write_text("1\n")
    node = tmp_path / "devices" / "system" / "node" / "node1"
    node.mkdir(parents=True)
    (node / "cpulist").write_text("64-127,192-255\n")
    n, cpus = hal.pci_numa_cpus("0000:C1:00.0", str(tmp_path))
    assert n == 1 and len(cpus) == 128 and cpus[0] == 64 and cpus[-1] == 255
    assert hal.pci_numa_cpus("0000:aa:00.0", str(tmp_path)) == (-1, [])         # unknown device
    (dev / "numa_node").write_text("-1\n")
    assert hal.pci_numa_cpus("0000:c1:00.0", str(tmp_path)) == (-1, [])         # the kernel reports no node


def test_a_current_build_is_used_without_writing_the_checkout(monkeypatch):
    """bench.py, smoke() and the tests may run under an account that cannot write the checkout it was built in: a build whose recorded
    tree digest is current is found without creating, truncating or locking any file."""
    import builtins
    from zeth_amd import build as b
    assert b.ensure_built(oracle=True) == b.LIB                       # current (the suite's conftest built it)
    real_open = builtins.open

    def read_only_open(path, mode="r", *a, **k):
        if any(c in mode for c in "wax+"):
            raise PermissionError(f"read-only checkout: {path}")
        return real_open(path, mode, *a, **k)

    def no_makedirs(*a, **k):
        raise PermissionError("read-only checkout")
    monkeypatch.setattr(builtins, "open", read_only_open)
    monkeypatch.setattr(os, "makedirs", no_makedirs)
    assert b.ensure_built(oracle=True) == b.LIB and b.ensure_built() == b.LIB
