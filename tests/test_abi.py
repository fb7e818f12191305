"""CPU: the C-ABI shared library loads (no GPU needed) and exports every symbol include/clipfsar_hip.h declares;
the ctypes signatures in clip_fsar_amd/hip.py have the arity of the header prototypes.  No compute calls."""
import os
import re

from _abi import _prototypes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "clipfsar_hip.h")


def _header_prototypes():
    return _prototypes(HEADER, "cfsar_")


def test_header_symbols_exported_and_arity_matches():
    import __graft_entry__ as ge
    ge.build()                                    # hipcc cross-compile (no-op when up to date) + load
    from clip_fsar_amd import hip
    L = hip.lib()
    protos = _header_prototypes()
    assert len(protos) == 48, protos
    for name, nargs in protos.items():
        assert hasattr(L, name), "symbol %s declared in the header is not exported" % name
        if name == "cfsar_last_error":
            continue
        assert name in hip.SIGNATURES, "no ctypes signature for %s" % name
        assert len(hip.SIGNATURES[name]) == nargs, (name, len(hip.SIGNATURES[name]), nargs)
    assert L.cfsar_version() >= 200
    assert isinstance(L.cfsar_last_error(), bytes)


def test_exported_symbols_are_exactly_the_header():
    """`nm -D` of the product build shows the header's entry points and nothing else of ours: no cfsar_debug_* hooks, no
    internal helpers, no kernel host stubs (built with -fvisibility=hidden; dev hooks live behind CFSAR_DEV=1 and
    include/clipfsar_hip_dev.h)."""
    import subprocess
    import __graft_entry__ as ge
    ge.build()
    from clip_fsar_amd import hip
    if os.environ.get("CFSAR_DEV", "0") == "1":
        import pytest
        pytest.skip("developer build")
    out = subprocess.run(["nm", "-D", "--defined-only", hip.LIB_PATH], stdout=subprocess.PIPE, text=True, check=True).stdout
    syms = {l.split()[-1] for l in out.splitlines() if l.strip()}
    ours = {s for s in syms if not s.startswith(("__hip", "_init", "_fini", "__bss", "_edata", "_end"))}
    assert ours == set(_header_prototypes()), sorted(ours ^ set(_header_prototypes()))
    assert not any("debug" in s for s in syms)


def test_dev_knobs_absent_from_product_sources():
    """The shipped kernels read no environment variables and carry no trace / stamp plumbing outside CFSAR_DEV blocks."""
    csrc = os.path.join(ROOT, "clip-fsar_amd", "csrc")
    for f in sorted(os.listdir(csrc)):
        text = open(os.path.join(csrc, f)).read()
        text = re.sub(r"#ifdef CFSAR_DEV.*?#endif", "", text, flags=re.S)
        assert "getenv" not in text, f
        assert "cfsar_debug_" not in text, f
        assert not re.search(r"\bstamp\(", text), f
        assert "static bool attr_set" not in text, f            # per-process flags for a per-device attribute


def test_argument_validation_without_gpu():
    """Entry points validate arguments before touching the device: bad shapes return an error code and a message."""
    from clip_fsar_amd import hip
    L = hip.lib()
    rc = L.cfsar_gemm(None, None, None, None, None, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0, 0, None)
    assert rc != 0 and b"null" in L.cfsar_last_error()
    rc = L.cfsar_layernorm(None, 4, None, 4, 0, None, None, 1, 4, 1e-5, None)
    assert rc != 0


def test_no_cpu_fallback_in_product_path():
    """The product path must not import the oracle or fall back to torch math: wrappers reject CPU tensors."""
    import pytest
    import torch
    from clip_fsar_amd import hip
    with pytest.raises(RuntimeError, match="HIP device tensor"):
        hip.layernorm(torch.zeros(4, 8), torch.zeros(4, 8), torch.ones(8), torch.zeros(8), 4, 8)
    pkg = os.path.join(ROOT, "clip-fsar_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith(".py"):
                src = open(os.path.join(dirpath, f)).read()
                assert "clipfsar_oracle" not in src and "ref_harness" not in src, os.path.join(dirpath, f)


def test_hot_kernels_keep_their_scratch_budgets():
    """Regression guard on the compiler's resource report (clip-fsar_amd/build.py writes build/resource_usage.json): the
    kernels of the ViT / RN50 hot path keep their working set in registers.  A run-time loop bound or a struct copy that
    sends an accumulator array to scratch is a 20-30 % slowdown that no parity test notices."""
    import json
    import __graft_entry__ as ge
    ge.build()
    from clip_fsar_amd import build as b
    if not os.path.exists(b.USAGE):
        b.build(force=True, verbose=False)
    usage = json.load(open(b.USAGE))
    assert len(usage) > 40, len(usage)
    hot = {  # substring of the mangled name -> max scratch bytes per lane
        "vit_attn_bf16_kernelIDF16bLi7ELi13ELi4ELi3E": 0, "vit_attn_bf16_kernelIDF16bLi9ELi17E": 0,
        "vit_attn_bf16_kernelIDF16_Li7ELi13ELi4ELi3E": 0, "vit_attn_bf16_kernelIDF16_Li9ELi17E": 0,      # the fp16 numerics mode
        "vit_gemm_kernelIDF16_DF16_Li0ELi1ELi2E": 0, "vit_gemm_kernelIDF16_DF16_Li0ELi2ELi2E": 0, "layernorm_kernel": 0,
        # fp16 c_fc (LN-fold + QuickGELU + per-frame fixed-point column sums, round 4): its 192-row form spills ONE epilogue register; what a
        # spill must never touch -- the destination of a compiler-invisible load before its wait -- is checked by tests/test_asm_audit.py
        "vit_gemm_kernelIDF16_DF16_Li1ELi2ELi2E": 16,
        # the persistent ViT GEMM (gemm_vit.hip): the LDS-DMA instances keep (nearly) everything in registers -- an LN-folded build
        # with 12 spilled registers returned stale lanes under a concurrent second stream (tests/test_gpu_kernels.py::
        # test_vit_gemms_are_bit_stable_under_a_second_stream), so these limits are tight on purpose; the register-staged long-K
        # instance (c_proj) spills tile-boundary values (never in the K loop)
        "vit_gemm_kernelIDF16bDF16bLi0ELi0ELi1E": 0, "vit_gemm_kernelIDF16bDF16_Li0ELi1ELi1E": 0,
        "vit_gemm_kernelIDF16_DF16bLi0ELi2ELi1E": 0, "vit_gemm_kernelIDF16_DF16bLi1ELi2ELi1E": 0,
        # round 3 product policy for K <= 1024: the LDS-DMA path with the pieces issued one barrier earlier (OPATH 2)
        "vit_gemm_kernelIDF16bDF16bLi0ELi0ELi2E": 0, "vit_gemm_kernelIDF16bDF16_Li0ELi1ELi2E": 0,
        "vit_gemm_kernelIDF16_DF16bLi0ELi2ELi2E": 0, "vit_gemm_kernelIDF16_DF16bLi1ELi2ELi2E": 0,
        "vit_gemm_kernelIDF16bDF16_Li0ELi1ELi0E": 128,
        # p12 (QKV, c_fc, out_proj / c_proj): a few loop-invariant epilogue scalars are spilled at kernel entry and reloaded
        # after the K loop (checked in the ISA: nothing inside the main loop); a main-loop spill would be hundreds of bytes
        # (round 3: 68 B without packed-fp32 VALU ops -- two more entry scalars)
        "gemm_kernel_p12IDF16bLi0ELb0E": 96, "gemm_kernel_p12IDF16bLi1ELb0E": 96, "gemm_kernel_p12IfLi0ELb1E": 128,
        "gemm_kernel_p12IDF16_Li0ELb1E": 128,              # fp16 residual stream (out_proj / c_proj of the bf16 mode)
        "gemm_kernel_p10IDF16bLi0ELb0ELb0ELb1E": 8, "gemm_kernel_p10IfLi0ELb1ELb0ELb1E": 8,      # RN50 implicit 3x3 convs, Cout > 128
        "gemm_kernel_p3IDF16bDF16bLi0ELb0ELb0ELb1ELb0E": 0, "gemm_kernel_p3IDF16bDF16bLi0ELb0ELb0ELb1ELb1E": 0,   # RN50 implicit convs
        # the RN50 tower's fp16 mode (round 4): the same kernels on IEEE-half operands keep the bf16 instances' budgets
        "gemm_kernel_p3IDF16_DF16_Li0ELb0ELb0ELb1ELb0E": 0, "gemm_kernel_p3IDF16_DF16_Li0ELb0ELb0ELb1ELb1E": 0,
        "gemm_kernel_p3IDF16_DF16_Li0ELb0ELb0ELb0ELb0E": 0, "gemm_kernel_p3IDF16_DF16_Li0ELb1ELb0ELb0ELb0E": 0,
        "gemm_kernel_p12IDF16_Li0ELb0ELb1EDF16_E": 96, "gemm_kernel_p12IDF16_Li0ELb1ELb1EDF16_E": 128, "gemm_kernel_p12IfLi0ELb0ELb1EDF16_E": 128,
        "gemm_kernel_p10IDF16_Li0ELb0ELb0ELb1EDF16_E": 16, "avgpool2_x8_kernelIDF16_E": 0, "stem_conv1_kernelIDF16_": 0,
        "stem_conv1_kernel": 0,
        "conv3x3_direct_kernelILi32ELi32E": 0, "conv3x3_direct_kernelILi32ELi64E": 0, "conv3x3_direct_kernelILi64ELi64E": 0,   # weights in registers
        "cos_otam_kernel": 0,                              # OTAM DP rows in registers (T = 8 / 16) or LDS (run-time T)
        "skinny_gemm_f32_kernel": 0,
    }
    for key, limit in hot.items():
        names = [n for n in usage if key in n]
        assert names, "kernel %s not found in the resource report" % key
        for n in names:
            assert usage[n].get("scratch", 0) <= limit, (n, usage[n])
    # the c_fc kernel (p6 + QuickGELU) and the main loops of the one-wave-per-SIMD family may spill a few epilogue scalars;
    # bound it so that a main-loop spill (hundreds of bytes) is caught
    for n, u in usage.items():
        if "gemm_kernel_p6" in n or "gemm_kernel_p10" in n or "gemm_kernel_p12" in n:
            assert u.get("scratch", 0) <= 256, (n, u)

