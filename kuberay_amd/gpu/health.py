"""GPU health gate: rocm-smi liveness + on-device gfx950 probes.

Backs the worker readiness probe injected by the pod builder
(``python -m kuberay_amd.gpu.probe``) and the GPU-gated sim-kubelet used in
``pytest -m gpu`` runs. The native extension is REQUIRED on GPU hosts — if
/dev/kfd exists and the extension is missing, this module raises instead of
silently passing (no silent eager fallback).
"""
from __future__ import annotations

import os
from dataclasses import dataclass
from typing import Dict, List, Optional

from . import rocm_smi

# Healthy MI355X streams ~6 TB/s; 1 TB/s floor catches an HBM stack or
# clock-park collapse without flaking on a busy GPU.
DEFAULT_HBM_FLOOR_GB_S = 1000.0


class GpuHealthError(RuntimeError):
    pass


def gpu_node() -> bool:
    """Is this host a ROCm GPU node?"""
    return os.path.exists("/dev/kfd")


def _load_native():
    try:
        from .._native import gpuhealth  # type: ignore
        return gpuhealth
    except ImportError as e:
        if gpu_node():
            raise GpuHealthError(
                "kuberay_amd._native.gpuhealth extension is not built on a GPU "
                "node — build it with `python -m kuberay_amd._native.build` "
                f"(import error: {e})") from e
        return None


@dataclass
class HealthReport:
    healthy: bool
    mfma_ok: Optional[bool] = None
    hbm_gb_s: Optional[float] = None
    rocm_smi_ok: Optional[bool] = None
    detail: str = ""
    # burn-in level only (check_gpu_burn_in); None from the quick/full gate
    mfma_exact: Optional[Dict[str, bool]] = None
    hbm_pattern_ok: Optional[bool] = None
    hbm_bytes_checked: Optional[int] = None
    hbm_flipped_bits: Optional[int] = None
    # CU sweep of the burn-in level; None when the native module has none
    cu_total: Optional[int] = None
    cu_covered: Optional[int] = None
    cu_faulty: Optional[List[str]] = None
    # MFMA load of the burn-in level; None unless it was asked for
    mfma_load_ok: Optional[bool] = None
    mfma_load_tflops: Optional[Dict[str, float]] = None
    mfma_load_clock_mhz: Optional[Dict[str, float]] = None
    mfma_load_faulty: Optional[List[str]] = None
    mfma_load_ok_by_dtype: Optional[Dict[str, bool]] = None


def _rocm_smi_ok() -> bool:
    try:
        return bool(rocm_smi.get_gpu_stats())
    except Exception:
        return False


def _gate_problems(result, hbm_floor_gb_s: float) -> list:
    """What the quick/full gate found wrong, one entry per failed check."""
    problems = []
    if not result["mfma_ok"]:
        problems.append("mfma_ok=False")
    if not result["hbm_ok"]:
        problems.append(f"hbm_gb_s={result['hbm_gb_s']:.0f} below the floor "
                        f"of {hbm_floor_gb_s:.0f}")
    return problems


def _hip_failure(error: RuntimeError, rocm_ok: bool) -> HealthReport:
    """A failing HIP call is the likeliest symptom of a wedged device: it is
    the gate's verdict, not a crash of the probe."""
    return HealthReport(healthy=False, rocm_smi_ok=rocm_ok, detail=str(error))


def check_gpu_health(device: int = 0, quick: bool = False,
                     hbm_floor_gb_s: float = DEFAULT_HBM_FLOOR_GB_S) -> HealthReport:
    """Full gate: rocm-smi responds AND the device executes MFMA AND streams
    HBM above the floor. Raises GpuHealthError on non-GPU hosts; ``detail``
    names what failed, a HIP error of the device included."""
    if not gpu_node():
        raise GpuHealthError("not a GPU node (/dev/kfd missing)")

    rocm_ok = _rocm_smi_ok()
    native = _load_native()
    if native.device_count() <= device:
        return HealthReport(healthy=False, rocm_smi_ok=rocm_ok,
                            detail=f"device {device} not visible to HIP")
    try:
        result = native.health_check(device, hbm_floor_gb_s, quick)
    except RuntimeError as e:
        return _hip_failure(e, rocm_ok)
    problems = _gate_problems(result, hbm_floor_gb_s)
    if not rocm_ok:
        problems.append("rocm-smi did not respond")
    return HealthReport(
        healthy=bool(result["healthy"]) and rocm_ok,
        mfma_ok=bool(result["mfma_ok"]),
        hbm_gb_s=float(result["hbm_gb_s"]),
        rocm_smi_ok=rocm_ok,
        detail="; ".join(problems),
    )


DEFAULT_BURN_IN_HBM_FRACTION = 0.9


def _cu_name(where, short: bool = False) -> str:
    if short:
        return f"xcc{where['xcc']}/se{where['se']}/cu{where['cu']}"
    return f"xcc{where['xcc']}/se{where['se']}/sh{where['sh']}/cu{where['cu']}"


def _cu_problem(where) -> str:
    """One faulty CU of the sweep: where, and what its LDS and SIMDs showed."""
    parts = []
    lds = where.get("lds") or {}
    if lds.get("bad_words"):
        parts.append(f"lds {lds['bad_words']} bad words mask "
                     f"0x{lds['bad_bit_mask']:08x} first word "
                     f"{lds['first_bad_word']}")
    for simd, dtype in where.get("mfma") or ():
        parts.append(f"mfma {dtype} on simd {simd}")
    return f"cu {_cu_name(where)}: " + "; ".join(parts)


MFMA_LOAD_DTYPES = ("bf16", "f16", "fp8", "mxfp4")
MAX_MFMA_LOAD_SECONDS = 60.0
# TFLOP/s floors of the MFMA load: half of the lowest 2 s run per data type on
# an MI355X, three runs on each of two nodes (2313 / 2330 / 2361 / 6783,
# docs/benchmarks.md "MFMA load"), rounded down to two digits. Half leaves room for the spread between
# devices, a busy neighbour and a power-capped clock; the collapse the floor is
# for (a parked engine clock) is several-fold.
DEFAULT_MFMA_FLOOR_TFLOPS = {"bf16": 1100.0, "f16": 1100.0, "fp8": 1100.0,
                             "mxfp4": 3300.0}


def _mfma_load(native, device: int, load_seconds: float, floors: Dict[str, float]):
    """The MFMA load, ``load_seconds / 4`` per data type. Returns (ok by data
    type, tflops, clock_mhz, faulty, problems)."""
    if not hasattr(native, "mfma_load"):
        return {}, {}, {}, [], ["mfma load: asked for, but this native module "
                                "has no mfma_load"]
    ok, tflops, clock, faulty, problems = {}, {}, {}, [], []
    for dtype in MFMA_LOAD_DTYPES:
        floor = float(floors[dtype])
        before = len(problems)
        r = native.mfma_load(device, dtype, seconds=load_seconds / len(MFMA_LOAD_DTYPES),
                             floor_tflops=floor)
        tflops[dtype], clock[dtype] = float(r["tflops"]), float(r["clock_mhz"])
        for f in r["faulty"]:
            faulty.append(f"{dtype} {_cu_name(f, short=True)} simd {f['simd']}")
            problems.append(f"mfma load {dtype}: cu {_cu_name(f)} simd {f['simd']}: "
                            f"{f['bad_elements']} bad elements")
        if tflops[dtype] < floor:
            problems.append(
                f"mfma load {dtype}: {tflops[dtype]:.0f} TFLOP/s below the floor of "
                f"{floor:.0f} (clock {clock[dtype]:.0f} MHz, "
                f"{float(r['cycles_per_mfma']):.1f} cycles/MFMA)")
        elif not r["ok"] and not r["faulty"]:
            problems.append(f"mfma load {dtype}: not ok")
        ok[dtype] = len(problems) == before
    return ok, tflops, clock, faulty, problems


def check_gpu_burn_in(device: int = 0,
                      hbm_fraction: float = DEFAULT_BURN_IN_HBM_FRACTION,
                      hbm_floor_gb_s: float = DEFAULT_HBM_FLOOR_GB_S,
                      require_cu_coverage: bool = False,
                      load_seconds: float = 0.0,
                      mfma_floor_tflops: Optional[Dict[str, float]] = None) -> HealthReport:
    """Burn-in level: the full gate of ``check_gpu_health``, then the exact
    MFMA verification on the bf16, f16, fp8 and MXFP4 data paths, then a
    data-verifying pattern sweep over ``hbm_fraction`` of the free HBM, then
    the CU sweep (LDS march on every CU, the exact MFMA tiles on every SIMD).
    A faulty CU is unhealthy and named in ``detail``; CUs the sweep did not
    reach are reported, and unhealthy only with ``require_cu_coverage``.
    With ``load_seconds > 0`` the MFMA load follows: every matrix pipe kept
    busy on self-checking data for a quarter of that time per data type. A
    wrong element, or a rate under ``mfma_floor_tflops`` (by data type, over
    ``DEFAULT_MFMA_FLOOR_TFLOPS``), is unhealthy and named in ``detail``.
    Raises GpuHealthError on non-GPU hosts; ``detail`` names what failed."""
    if not gpu_node():
        raise GpuHealthError("not a GPU node (/dev/kfd missing)")
    if not 0.0 < hbm_fraction <= 1.0:
        raise ValueError(f"hbm_fraction must be in (0, 1], got {hbm_fraction}")
    if not 0.0 <= load_seconds <= MAX_MFMA_LOAD_SECONDS:
        raise ValueError(f"load_seconds must be in [0, {MAX_MFMA_LOAD_SECONDS:.0f}], "
                         f"got {load_seconds}")
    floors = dict(DEFAULT_MFMA_FLOOR_TFLOPS)
    for dtype, floor in (mfma_floor_tflops or {}).items():
        if dtype not in floors or not float(floor) >= 0.0:
            raise ValueError(f"mfma_floor_tflops: {dtype}={floor} is not a data type of "
                             f"{MFMA_LOAD_DTYPES} with a floor of at least 0")
        floors[dtype] = float(floor)

    rocm_ok = _rocm_smi_ok()
    native = _load_native()
    if native.device_count() <= device:
        return HealthReport(healthy=False, rocm_smi_ok=rocm_ok,
                            detail=f"device {device} not visible to HIP")
    try:
        result = native.burn_in(device, hbm_fraction, hbm_floor_gb_s)
    except RuntimeError as e:
        return _hip_failure(e, rocm_ok)
    pattern = result["hbm_pattern"]
    exact = {k: bool(v) for k, v in result["mfma_exact"].items()}

    problems = _gate_problems(result, hbm_floor_gb_s)
    for dtype, ok in exact.items():
        if not ok:
            wg, row, col, got, expected = result["mfma_first_bad"][dtype]
            problems.append(f"mfma {dtype}: tile {wg} [{row}][{col}] "
                            f"got {got!r} expected {expected!r}")
    if not result["hbm_pattern_ok"]:
        problems.append(
            f"hbm pattern: {pattern['mismatched_words']} bad words, "
            f"{pattern['flipped_bits']} flipped bits, mask "
            f"0x{pattern['bad_bit_mask']:08x}, first bad offset "
            f"{pattern['first_bad_offset']}")
    # a native module without the CU sweep gives the report it always gave
    sweep = result.get("cu_sweep")
    healthy = bool(result["healthy"])
    cu_total = cu_covered = cu_faulty = None
    if sweep is not None:
        cu_total, cu_covered = int(sweep["cu_total"]), int(sweep["cu_covered"])
        cu_faulty = [_cu_name(f, short=True) for f in sweep["faulty"]]
        problems.extend(_cu_problem(f) for f in sweep["faulty"])
        healthy = healthy and bool(result.get("cu_ok", not cu_faulty))
        if not result.get("cu_coverage_complete", cu_covered >= cu_total):
            problems.append(f"cu coverage {cu_covered}/{cu_total} after "
                            f"{sweep['rounds']} rounds")
            healthy = healthy and not require_cu_coverage
    load_ok = load_by_dtype = load_tflops = load_clock = load_faulty = None
    if load_seconds > 0.0:
        try:
            load_by_dtype, load_tflops, load_clock, load_faulty, load_problems = _mfma_load(
                native, device, load_seconds, floors)
        except RuntimeError as e:
            return _hip_failure(e, rocm_ok)
        problems.extend(load_problems)
        load_ok = not load_problems
        healthy = healthy and load_ok
    if not rocm_ok:
        problems.append("rocm-smi did not respond")
    return HealthReport(
        healthy=healthy and rocm_ok,
        mfma_ok=bool(result["mfma_ok"]),
        hbm_gb_s=float(result["hbm_gb_s"]),
        rocm_smi_ok=rocm_ok,
        detail="; ".join(problems),
        cu_total=cu_total, cu_covered=cu_covered, cu_faulty=cu_faulty,
        mfma_exact=exact,
        hbm_pattern_ok=bool(result["hbm_pattern_ok"]),
        hbm_bytes_checked=int(pattern["bytes_checked"]),
        hbm_flipped_bits=int(pattern["flipped_bits"]),
        mfma_load_ok=load_ok, mfma_load_tflops=load_tflops,
        mfma_load_clock_mhz=load_clock, mfma_load_faulty=load_faulty,
        mfma_load_ok_by_dtype=load_by_dtype,
    )


def sim_kubelet_gpu_gate(pod: dict) -> bool:
    """gpu_gate hook for SimKubelet: a GPU-requesting pod only turns Ready if
    the local MI355X passes the quick health gate. Whatever the check raises
    is a failed gate: a pod must never turn Ready because the probe crashed."""
    try:
        return check_gpu_health(quick=True).healthy
    except Exception:
        return False
