"""The C-ABI library loads without a GPU and exports exactly what include/pcc_hip.h declares."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_symbols():
    text = open(os.path.join(ROOT, "include", "pcc_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(pcc_[a-z0-9_]+)\s*\(", text)))


def test_every_declared_symbol_is_exported_and_bound(pcc):
    from pcc_amd import _lib
    L = pcc.lib()
    names = declared_symbols()
    assert len(names) >= 30
    for n in names:
        assert hasattr(L, n), f"{n} declared in pcc_hip.h but not exported by libpcc_hip.so"
        assert n in _lib.SIGNATURES, f"{n} has no ctypes signature in _lib.py"
    assert sorted(_lib.SIGNATURES) == names, set(_lib.SIGNATURES) ^ set(names)


def test_no_torch_types_in_header():
    text = open(os.path.join(ROOT, "include", "pcc_hip.h")).read()
    assert 'extern "C"' in text
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)          # signatures only, comments stripped
    assert "torch" not in code.lower() and "at::" not in code and "Tensor" not in code
    assert "#include <stdint.h>" in code and code.count("#include") == 1


def test_host_entry_points_without_gpu(pcc):
    L = pcc.lib()
    assert L.pcc_version() >= 1
    assert L.pcc_hash_capacity(1000) == 2048 and L.pcc_hash_capacity(3) == 1024
    assert L.pcc_scan_scratch_elems(5000) >= 2 * 5000
    assert L.pcc_conv_packed_elems(27, 128, 3) == 27 * 128 * 32
    assert L.pcc_topk_state_elems(2) >= 2 * 259
    # the thresholds of the small-launch paths are host state: defaults, set / read back, restore
    assert L.pcc_small_map_max() in (0, 256)
    was = L.pcc_conv_small_max(-1)
    assert was == 640 or os.environ.get("PCC_CONV_SMALL_MAX")
    assert L.pcc_conv_small_max(17) == was and L.pcc_conv_small_max(was) == 17 and L.pcc_conv_small_max(-1) == was
    paths = L.pcc_small_paths(-1)
    assert 0 <= paths <= 7
    assert L.pcc_small_paths(2) == paths and L.pcc_small_paths(paths) == 2 and L.pcc_small_paths(-1) == paths
    # error path: message available, no exception across the ABI
    pmf = np.array([-1.0, 2.0], dtype=np.float32)
    cdf = np.zeros(3, dtype=np.int32)
    rc = L.pcc_pmf_to_quantized_cdf(pmf.ctypes.data, 2, 16, cdf.ctypes.data)
    assert rc < 0 and b"pmf" in L.pcc_last_error()


def test_header_parser_on_planted_text():
    """parse_header on two prototypes that cover every mapped type: a multi-line parameter list, a (void) list, a const char*
    return; comments and preprocessor lines are dropped, integer PCC_* defines collected"""
    from ctypes import c_char_p, c_float, c_int, c_int32, c_int64, c_void_p
    from pcc_amd import _lib
    text = """
    /* a comment with a prototype in it: int pcc_not_this(int a); */
    #include <stdint.h>
    #define PCC_PLANTED 7
    #define PCC_PLANTED_NEG (-5)   /* trailing comment */
    #define PCC_NOT_AN_INT 1.5f
    extern "C" {
    const char* pcc_planted_name(void);
    int64_t pcc_planted(int dev, int32_t a, int64_t n,
                        float half, char* out, const char *name,
                        const uint64_t* keys, double * normals,
                        void* stream);
    }
    """
    protos, consts = _lib.parse_header(text)
    assert protos == {
        "pcc_planted_name": (c_char_p, []),
        "pcc_planted": (c_int64, [("dev", c_int), ("a", c_int32), ("n", c_int64), ("half", c_float), ("out", c_char_p),
                                  ("name", c_char_p), ("keys", c_void_p), ("normals", c_void_p), ("stream", c_void_p)]),
    }
    assert consts == {"PLANTED": 7, "PLANTED_NEG": -5}


def test_header_parser_never_guesses():
    from pcc_amd import _lib
    for bad in ("int pcc_planted(const float* x, size_t n);", "size_t pcc_planted(void);", "int pcc_planted(float** rows);",
                "int pcc_planted(int32_t);", "struct pcc_thing { int a };"):
        with pytest.raises(ValueError):
            _lib.parse_header(bad)


def test_wrong_argument_count_raises(pcc):
    """a surplus or a missing argument is a TypeError before the call (host-only entry points: nothing is launched)"""
    L = pcc.lib()
    buf = ctypes.create_string_buffer(128)
    with pytest.raises(TypeError):
        L.pcc_hash_capacity(1000, 0)
    with pytest.raises(TypeError):
        L.pcc_conv_kernel_name(0, 1000, 128, 128, 1000, 27, 1, buf, 128, 0)
    with pytest.raises(TypeError):
        L.pcc_hash_capacity()
    assert L.pcc_hash_capacity(1000) == 2048
    assert L.pcc_conv_kernel_name(0, 1000, 128, 128, 1000, 27, 1, buf, 128) == 0 and buf.value == b"conv_small_kernel<4, 3>"


def test_constants_come_from_the_header(pcc):
    import importlib
    from pcc_amd import _lib, augment, render, sparse
    voxelize = importlib.import_module("pcc_amd.voxelize")          # (the package exports the function under the module's name)
    P = _lib.PCC
    assert (P.OK, P.COORD_LIMIT, P.BATCH_LIMIT, P.COUNT_ERR_RANGE, P.ERR_UNSUPPORTED, P.ACT_LEAKY_RELU) == (0, 130000, 1022, -2, -3, 2)
    assert (sparse.ACT_NONE, sparse.ACT_RELU, sparse.ACT_LRELU, sparse.COUNT_ERR_RANGE) == (0, 1, 2, -2)
    assert augment.BATCH_SLOTS == 1023 and render.COORD_LIMIT == 130000 and voxelize.COORD_LIMIT == 130000


def test_product_never_imports_the_oracle():
    pkg = os.path.join(ROOT, "learned-compression-of-point-cloud-geometry-and-attributes_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".cpp", ".h")):
                src = open(os.path.join(dirpath, f)).read()
                assert not re.search(r"^\s*(from|import)\s+oracle\b", src, flags=re.M), f
                assert "oracle/" not in src or f.endswith(".md"), f


def test_bench_uses_the_oracle_only_in_its_cpu_baseline_leg():
    src = open(os.path.join(ROOT, "bench.py")).read()
    body = src.split("def cpu_baseline(")[1].split("\ndef main(")[0]
    rest = src.replace(body, "")
    assert "oracle" in body
    assert not re.search(r"^\s*(from|import)\s+oracle\b", rest, flags=re.M)


def test_build_checks_of_the_convolution_kernels(pcc):
    """build() fails when an MFMA convolution kernel uses scratch or spills (the compiler's resource remarks), and when the
    code generated for conv_small_kernel touches a register an inline-assembly LDS read is still filling: both
    checks pass on the built library, and the lint catches a planted violation"""
    from pcc_amd import _lib
    res = _lib.check_kernel_resources()
    assert any("conv_small_kernel" in k for k in res) and all(v[1] in (0, None) for v in res.values())
    assert _lib.check_small_kernel_lds_reads() > 50
    good = """
0000000000001000 <_ZN3pcc17conv_small_kernelILi1ELi8EEEvNS_8ConvArgsE>:
	ds_read_b128 v[14:17], v8                                  // 000000032A64: D9FE0000
	v_mfma_f32_16x16x4_f32 v[0:3], v40, v41, v[0:3]            // 000000032A6C: D3C50000
	s_waitcnt lgkmcnt(0)                                       // 000000032B64: BF8CC07F
	v_cndmask_b32_e64 v40, v14, v15, s[4:5]                    // 000000032B68: D1000028
	s_endpgm
"""
    assert _lib.lint_lds_reads(good) == 1
    bad = good.replace("v_mfma_f32_16x16x4_f32 v[0:3], v40, v41, v[0:3]", "v_mov_b32_e32 v90, v15")
    import pytest
    with pytest.raises(RuntimeError, match="still in flight"):
        _lib.lint_lds_reads(bad)


# (cin, cout, n_out, has_nbr) -> the kernel pcc_conv_fwd launches (K = 27 with a map, else 1 and n_in = n_out)
_FP32_PLANS = [
    (128, 128, 1_000, True, "conv_small_kernel<4, 3>"),
    (64, 64, 5_000, True, "conv_small_kernel<2, 3>"),
    (96, 32, 3_000, True, "conv_small_kernel<1, 8>"),
    (128, 128, 30_000, True, "conv_mfma_buf_kernel<64, 64, 2, 2, 4, true>"),
    (96, 128, 20_000, True, "conv_mfma_buf_kernel<64, 64, 2, 2, 3, true>"),
    (128, 128, 72_000, True, "conv_mfma_buf_kernel<32, 128, 1, 4, 4, true>"),
    (128, 128, 1_263_766, True, "conv_mfma_buf_kernel<64, 128, 2, 2, 4, true>"),
    (64, 64, 5_160_000, True, "conv_mfma_buf_kernel<128, 64, 2, 2, 2, true>"),
    (32, 32, 200_000, True, "conv_mfma_buf_kernel<128, 32, 4, 1, 1, true>"),
    (128, 128, 100_000, False, "conv_mfma_buf_kernel<32, 128, 1, 4, 4, false>"),
    (3, 8, 50_000, True, "conv_thin_kernel<3, 8>"),
    (2, 6, 700, True, "conv_thin_kernel<2, 2>"),
]


def test_conv_kernel_name_follows_the_launch_plan(pcc):
    """pcc_conv_kernel_name: the kernel and template parameters each mode's launch runs (csrc/conv.hip, plan_conv), on the host"""
    import ctypes
    L = pcc.lib()

    def name(mode, cin, cout, n_out, has_nbr=True, n_in=None, K=None):
        buf = ctypes.create_string_buffer(128)
        rc = L.pcc_conv_kernel_name(mode, n_out if n_in is None else n_in, cin, cout, n_out, (27 if has_nbr else 1) if K is None else K,
                                    int(has_nbr), buf, len(buf))
        return buf.value.decode() if rc == 0 else rc

    for cin, cout, n_out, has_nbr, want in _FP32_PLANS:
        assert name(0, cin, cout, n_out, has_nbr) == want, (cin, cout, n_out, has_nbr)
    # bf16: chunks of 64 channels, never the small kernel; x3: 64 x 64 tiles for 64-wide outputs, nothing for 32-wide ones
    assert name(1, 128, 128, 1_000) == "conv_mfma_buf_kernel[bf16]<64, 64, 2, 2, 2, true>"
    assert name(1, 128, 128, 1_263_766) == "conv_mfma_buf_kernel[bf16]<64, 128, 2, 2, 2, true>"
    assert name(1, 256, 64, 5_160_000) == "conv_mfma_buf_kernel[bf16]<128, 64, 2, 2, 4, true>"
    assert name(1, 64, 32, 200_000) == "conv_mfma_buf_kernel[bf16]<128, 32, 4, 1, 1, true>"
    assert name(1, 128, 128, 72_000, has_nbr=False) == "conv_mfma_buf_kernel[bf16]<64, 128, 2, 2, 2, false>"
    assert name(2, 128, 128, 1_000) == "conv_mfma_buf_kernel[x3]<64, 64, 2, 2, 4, true>"
    assert name(2, 128, 128, 72_000) == "conv_mfma_buf_kernel[x3]<64, 128, 2, 2, 4, true>"
    assert name(2, 64, 64, 5_160_000) == "conv_mfma_buf_kernel[x3]<64, 64, 2, 2, 2, true>"
    assert name(2, 96, 64, 5_000) == "conv_mfma_buf_kernel[x3]<64, 64, 2, 2, 3, true>"
    unsupported = -3                                                # PCC_ERR_UNSUPPORTED
    for mode, cin, cout in ((2, 64, 32), (2, 64, 96), (1, 96, 128), (1, 3, 8), (2, 3, 8), (1, 512, 128), (0, 5, 8), (0, 288, 64)):
        assert name(mode, cin, cout, 10_000) == unsupported, (mode, cin, cout)
    # operands past the 32-bit buffer offsets: the 64-bit-addressed kernel in fp32, nothing in bf16 / x3
    assert name(0, 128, 64, 9_000_000) == "conv_mfma_kernel<128, 64, 2, 2, true>"
    assert name(0, 128, 128, 9_000_000, has_nbr=False) == "conv_mfma_kernel<64, 128, 2, 2, false>"
    assert name(0, 128, 128, 500, n_in=9_000_000) == "conv_mfma_kernel<64, 64, 2, 2, true>"
    assert name(1, 256, 128, 9_000_000) == unsupported and name(2, 128, 128, 9_000_000) == unsupported
    assert name(1, 128, 128, 45_000_000, n_in=1_000_000) == unsupported      # the map alone: n_out * K * 4 bytes
    assert name(0, 128, 128, 10_000, has_nbr=False, n_in=5_000) < 0    # no map: one row per input row
    # the small-kernel threshold is host state the plan reads
    was = L.pcc_conv_small_max(0)
    try:
        assert name(0, 128, 128, 1_000) == "conv_mfma_buf_kernel<64, 64, 2, 2, 4, true>"
        L.pcc_conv_small_max(64)
        assert name(0, 128, 128, 500) == "conv_small_kernel<4, 3>" and name(0, 128, 128, 600).startswith("conv_mfma_buf_kernel")
        assert name(0, 64, 64, 1_000) == "conv_small_kernel<2, 3>"          # 32 x 32 tiles x 2 for outputs below 128 wide
    finally:
        L.pcc_conv_small_max(was)
    assert name(0, 128, 128, 1_000) == "conv_small_kernel<4, 3>"
    # a buffer too short for the name is an argument error, not a truncated name
    assert L.pcc_conv_kernel_name(0, 1000, 128, 128, 1000, 27, 1, ctypes.create_string_buffer(8), 8) == -1
