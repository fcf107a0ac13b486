"""Readiness-probe CLI: ``python -m kuberay_amd.gpu.probe [--quick] [--device N]``.

Injected into GPU worker readiness probes by the pod builder
(common/pod.py init_liveness_and_readiness_probe). Exit 0 = healthy.

``--deep [--hbm-fraction F] [--require-cu-coverage]`` runs the burn-in level
instead (HBM pattern sweep + exact MFMA checks + the per-CU sweep of LDS and
SIMDs; with the flag, a CU the sweep could not reach fails it); the pod
builder injects it as a startupProbe on GPU workers whose template carries
``amd.com/gpu-burn-in: "true"``.

``--deep --load-seconds S [--mfma-floor-tflops DTYPE=N ...]`` adds the MFMA
load to the burn-in level: S seconds of self-checking MFMA on every matrix
pipe, a quarter per data type, with a TFLOP/s floor (annotation
``amd.com/gpu-burn-in-load-seconds``). Its fields appear in the output only
when it ran.
"""
from __future__ import annotations

import argparse
import json
import sys

from .health import (DEFAULT_BURN_IN_HBM_FRACTION, MAX_MFMA_LOAD_SECONDS,
                     MFMA_LOAD_DTYPES, GpuHealthError, check_gpu_burn_in,
                     check_gpu_health)


def main(argv=None) -> int:
    parser = argparse.ArgumentParser(description="MI355X GPU health probe")
    parser.add_argument("--quick", action="store_true",
                        help="fast gate for readiness probes (<~100 ms)")
    parser.add_argument("--device", type=int, default=0)
    parser.add_argument("--hbm-floor-gb-s", type=float, default=1000.0)
    parser.add_argument("--json", action="store_true", dest="json_out")
    parser.add_argument("--deep", action="store_true",
                        help="burn-in level: data-verifying HBM sweep and "
                             "exact MFMA checks (seconds, for startup probes)")
    parser.add_argument("--hbm-fraction", type=float,
                        default=DEFAULT_BURN_IN_HBM_FRACTION,
                        help="with --deep: fraction of the free HBM to sweep")
    parser.add_argument("--require-cu-coverage", action="store_true",
                        help="with --deep: unhealthy unless the CU sweep "
                             "reached every CU of the device")
    parser.add_argument("--load-seconds", type=float, default=0.0,
                        help="with --deep: seconds of self-checking MFMA load, "
                             "a quarter per data type (0: none, at most 60)")
    parser.add_argument("--mfma-floor-tflops", action="append", default=[],
                        metavar="DTYPE=N",
                        help="with --load-seconds: TFLOP/s floor of one data "
                             "type (bf16, f16, fp8, mxfp4); may be repeated")
    args = parser.parse_args(argv)
    if args.load_seconds and not args.deep:
        parser.error("--load-seconds needs --deep")
    if args.mfma_floor_tflops and not args.load_seconds:
        parser.error("--mfma-floor-tflops needs --load-seconds")
    load = {}
    if args.load_seconds:
        # the load's own arguments are refused here, as usage errors; the
        # plain --deep path is as it was
        if not 0.0 < args.load_seconds <= MAX_MFMA_LOAD_SECONDS:
            parser.error(f"--load-seconds must be in (0, {MAX_MFMA_LOAD_SECONDS:.0f}]")
        floors = {}
        for item in args.mfma_floor_tflops:
            dtype, sep, value = item.partition("=")
            try:
                floors[dtype] = float(value)
            except ValueError:
                sep = ""
            if not sep or dtype not in MFMA_LOAD_DTYPES or not floors[dtype] >= 0.0:
                parser.error(f"--mfma-floor-tflops wants DTYPE=N with DTYPE one of "
                             f"{', '.join(MFMA_LOAD_DTYPES)} and N >= 0, got {item!r}")
        load = {"load_seconds": args.load_seconds, "mfma_floor_tflops": floors or None}

    try:
        if args.deep:
            report = check_gpu_burn_in(device=args.device,
                                       hbm_fraction=args.hbm_fraction,
                                       hbm_floor_gb_s=args.hbm_floor_gb_s,
                                       require_cu_coverage=args.require_cu_coverage,
                                       **load)
        else:
            report = check_gpu_health(device=args.device, quick=args.quick,
                                      hbm_floor_gb_s=args.hbm_floor_gb_s)
    except GpuHealthError as e:
        print(f"gpu probe error: {e}", file=sys.stderr)
        return 2
    if args.deep:
        # the CU sweep's fields appear when the native module ran one
        swept = report.cu_total is not None
        # and the MFMA load's when it was asked for
        loaded = report.mfma_load_ok is not None
        if args.json_out:
            out = {
                "healthy": report.healthy, "mfma_ok": report.mfma_ok,
                "hbm_gb_s": report.hbm_gb_s, "rocm_smi_ok": report.rocm_smi_ok,
                "detail": report.detail, "mfma_exact": report.mfma_exact,
                "hbm_pattern_ok": report.hbm_pattern_ok,
                "hbm_bytes_checked": report.hbm_bytes_checked,
                "hbm_flipped_bits": report.hbm_flipped_bits}
            if swept:
                out.update(cu_total=report.cu_total, cu_covered=report.cu_covered,
                           cu_faulty=report.cu_faulty)
            if loaded:
                out.update(mfma_load_ok=report.mfma_load_ok,
                           mfma_load_tflops=report.mfma_load_tflops,
                           mfma_load_clock_mhz=report.mfma_load_clock_mhz,
                           mfma_load_faulty=report.mfma_load_faulty)
            print(json.dumps(out))
        else:
            cu = (f" cu_total={report.cu_total} cu_covered={report.cu_covered} "
                  f"cu_faulty={report.cu_faulty}") if swept else ""
            if loaded:
                cu += (f" mfma_load_ok={report.mfma_load_ok} "
                       f"mfma_load_tflops={report.mfma_load_tflops} "
                       f"mfma_load_clock_mhz={report.mfma_load_clock_mhz} "
                       f"mfma_load_faulty={report.mfma_load_faulty}")
            print(f"healthy={report.healthy} mfma_ok={report.mfma_ok} "
                  f"hbm_gb_s={report.hbm_gb_s} rocm_smi_ok={report.rocm_smi_ok} "
                  f"mfma_exact={report.mfma_exact} "
                  f"hbm_pattern_ok={report.hbm_pattern_ok} "
                  f"hbm_bytes_checked={report.hbm_bytes_checked} "
                  f"hbm_flipped_bits={report.hbm_flipped_bits}{cu}")
            if report.detail:
                print(report.detail, file=sys.stderr)
        return 0 if report.healthy else 1
    if args.json_out:
        print(json.dumps({
            "healthy": report.healthy, "mfma_ok": report.mfma_ok,
            "hbm_gb_s": report.hbm_gb_s, "rocm_smi_ok": report.rocm_smi_ok,
            "detail": report.detail}))
    else:
        print(f"healthy={report.healthy} mfma_ok={report.mfma_ok} "
              f"hbm_gb_s={report.hbm_gb_s} rocm_smi_ok={report.rocm_smi_ok}")
        if report.detail:
            print(report.detail, file=sys.stderr)
    return 0 if report.healthy else 1


if __name__ == "__main__":
    sys.exit(main())
