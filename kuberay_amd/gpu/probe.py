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

``--deep --gemm`` adds the GEMM check (annotation
``amd.com/gpu-burn-in-gemm``): one exact bf16 and one exact f16 GEMM through
direct-to-LDS loads, transposed LDS reads and MFMA, milliseconds long. Its
fields appear in the output only when it was asked for.

``--deep --gemm-narrow`` adds the narrow GEMM check (annotation
``amd.com/gpu-burn-in-gemm-narrow``): the same for fp8 and MXFP4, through the
8-bit and 4-bit transposed LDS reads with the MX scales from device memory.
Its fields follow those of ``--gemm``.

``--deep --attention`` adds the attention check (annotation
``amd.com/gpu-burn-in-attention``): one exact bf16 and one exact f16 attention
forward with online softmax. Its fields follow those of the GEMM checks.

``--deep --attention-causal`` adds the causal attention check (annotation
``amd.com/gpu-burn-in-attention-causal``): the same forward for many heads at
head dimension 128 under the causal mask. Its fields follow those of
``--attention``.

``--deep --attention-decode`` adds the decode attention check (annotation
``amd.com/gpu-burn-in-attention-decode``): one query token a sequence over a
paged KV cache, grouped-query heads, split-KV with a merge kernel. Its fields
follow those of ``--attention-causal``.

``--deep --moe`` adds the MoE check (annotation ``amd.com/gpu-burn-in-moe``):
the routed grouped GEMM of a mixture-of-experts layer with its top-k combine
by fp32 atomics. Its fields follow those of ``--attention-decode``.
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
    parser.add_argument("--gemm", action="store_true",
                        help="with --deep: the exact GEMM check through "
                             "direct-to-LDS loads and transposed LDS reads")
    parser.add_argument("--gemm-narrow", action="store_true",
                        help="with --deep: the exact fp8 and MXFP4 GEMM check "
                             "through the 8-bit and 4-bit transposed LDS reads")
    parser.add_argument("--attention", action="store_true",
                        help="with --deep: the exact attention check, online "
                             "softmax between two MFMAs")
    parser.add_argument("--attention-causal", action="store_true",
                        help="with --deep: the exact causal attention check, "
                             "many heads at head dimension 128")
    parser.add_argument("--attention-decode", action="store_true",
                        help="with --deep: the exact decode attention check, "
                             "paged KV cache, GQA and split-KV")
    parser.add_argument("--moe", action="store_true",
                        help="with --deep: the exact MoE check, routed grouped "
                             "GEMM and atomic scatter-add")
    args = parser.parse_args(argv)
    if args.gemm and not args.deep:
        parser.error("--gemm needs --deep")
    if args.gemm_narrow and not args.deep:
        parser.error("--gemm-narrow needs --deep")
    if args.attention and not args.deep:
        parser.error("--attention needs --deep")
    if args.attention_causal and not args.deep:
        parser.error("--attention-causal needs --deep")
    if args.attention_decode and not args.deep:
        parser.error("--attention-decode needs --deep")
    if args.moe and not args.deep:
        parser.error("--moe needs --deep")
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
    if args.gemm:
        load["gemm"] = True
    if args.gemm_narrow:
        load["gemm_narrow"] = True
    if args.attention:
        load["attention"] = True
    if args.attention_causal:
        load["attention_causal"] = True
    if args.attention_decode:
        load["attention_decode"] = True
    if args.moe:
        load["moe"] = True

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
            if args.gemm:
                out.update(gemm_exact=report.gemm_exact, gemm_faulty=report.gemm_faulty)
            if args.gemm_narrow:
                out.update(gemm_narrow_exact=report.gemm_narrow_exact,
                           gemm_narrow_faulty=report.gemm_narrow_faulty)
            if args.attention:
                out.update(attn_exact=report.attn_exact, attn_faulty=report.attn_faulty)
            if args.attention_causal:
                out.update(attn_causal_exact=report.attn_causal_exact,
                           attn_causal_faulty=report.attn_causal_faulty)
            if args.attention_decode:
                out.update(attn_decode_exact=report.attn_decode_exact,
                           attn_decode_faulty=report.attn_decode_faulty)
            if args.moe:
                out.update(moe_exact=report.moe_exact, moe_faulty=report.moe_faulty)
            print(json.dumps(out))
        else:
            cu = (f" cu_total={report.cu_total} cu_covered={report.cu_covered} "
                  f"cu_faulty={report.cu_faulty}") if swept else ""
            if loaded:
                cu += (f" mfma_load_ok={report.mfma_load_ok} "
                       f"mfma_load_tflops={report.mfma_load_tflops} "
                       f"mfma_load_clock_mhz={report.mfma_load_clock_mhz} "
                       f"mfma_load_faulty={report.mfma_load_faulty}")
            if args.gemm:
                cu += f" gemm_exact={report.gemm_exact} gemm_faulty={report.gemm_faulty}"
            if args.gemm_narrow:
                cu += (f" gemm_narrow_exact={report.gemm_narrow_exact} "
                       f"gemm_narrow_faulty={report.gemm_narrow_faulty}")
            if args.attention:
                cu += f" attn_exact={report.attn_exact} attn_faulty={report.attn_faulty}"
            if args.attention_causal:
                cu += (f" attn_causal_exact={report.attn_causal_exact} "
                       f"attn_causal_faulty={report.attn_causal_faulty}")
            if args.attention_decode:
                cu += (f" attn_decode_exact={report.attn_decode_exact} "
                       f"attn_decode_faulty={report.attn_decode_faulty}")
            if args.moe:
                cu += f" moe_exact={report.moe_exact} moe_faulty={report.moe_faulty}"
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
