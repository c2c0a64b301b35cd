"""CPU: the C-ABI shared library builds for gfx950, loads without a GPU and exports every symbol
include/pie_hip.h declares (no compute calls here)."""
import ctypes
import re
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent


def declared_symbols():
    text = (ROOT / "include" / "pie_hip.h").read_text()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(pie_[a-z0-9_]+)\s*\(", text)))


def test_library_builds_and_exports_header_symbols():
    from proxy_inference_engine_amd import _ffi, build
    lib_path = build.build()
    assert lib_path.exists()
    lib = ctypes.CDLL(str(lib_path))
    syms = declared_symbols()
    assert len(syms) >= 25 and "pie_qgemv_w4g64" in syms and "pie_decoder_step" in syms
    missing = [s for s in syms if not hasattr(lib, s)]
    assert not missing, f"declared in include/pie_hip.h but not exported: {missing}"
    assert sorted(_ffi.EXPORTS) == syms, "the ctypes binding and the header list different entry points"


def test_hello_and_size_helpers_without_gpu():
    from proxy_inference_engine_amd import _ffi
    import proxy_inference_engine
    assert proxy_inference_engine.pie_core.hello() == "pie_core ✓"      # tests/python/test_basic.py:16 of the reference
    lib = _ffi.load()
    assert lib.pie_version().startswith(b"pie_hip")
    assert lib.pie_w4s_bytes(4096, 4096) == 2048 * 2 * 2304                # pairs x slices x unit
    assert lib.pie_w4s_bytes(4096, 14336) == 2048 * 7 * 2304
    assert lib.pie_w4s_bytes(3, 4096) == 0 and lib.pie_w4s_bytes(4, 100) == 0
    n = (4 + 2 * 2) * 64
    arr = (ctypes.c_int32 * n)()
    assert lib.pie_qkv_row_map(4, 2, 64, arr) == 0
    m = list(arr)
    assert sorted(m) == list(range(n)) and m[:4] == [0, 32, 1, 33] and m[-1] == n - 1
    assert lib.pie_qkv_row_map(4, 2, 63, arr) != 0 and b"pie_qkv_row_map" in lib.pie_last_error()


def test_shape_errors_come_before_any_planning_without_gpu():
    """Entry points must refuse a bad shape with PIE_E_SHAPE before any plan or workspace arithmetic (a host-side division by zero in
    the many-row int4 GEMM's plan for N < 32 was a SIGFPE, not an error code)."""
    from proxy_inference_engine_amd import _ffi
    lib = _ffi.load()
    buf = ctypes.create_string_buffer(4096)
    p = ctypes.cast(buf, ctypes.c_void_p)
    for M, N, K in ((64, 16, 256), (64, 48, 256), (64, 64, 100), (0, 64, 256), (4, 16, 256)):
        rc = lib.pie_qgemm_w4m(p, p, M, N, K, _ffi.PIE_BF16, p, None)
        assert rc == -2 and b"pie_qgemm_w4m" in lib.pie_last_error(), (M, N, K, rc)


def test_product_never_imports_the_oracle():
    bad = []
    for f in (ROOT / "proxy_inference_engine_amd").rglob("*"):
        if f.suffix in (".py", ".hip", ".hpp", ".cpp", ".h") and "oracle" in f.read_text(errors="ignore").replace("the oracle", ""):
            if re.search(r"(import|from|include|CDLL).*oracle", f.read_text(errors="ignore")):
                bad.append(str(f))
    assert not bad, bad


def test_no_library_gemm_behind_the_c_abi():
    """Every GEMM on the path is hand-written (round 5 removed the hipBLASLt dlopen of rounds 1-4): the built library neither names nor
    links a BLAS, and the sources hold no include of one.  Size helpers of the 16-bit tile format answer without a GPU."""
    import subprocess
    from proxy_inference_engine_amd import _ffi, build
    blob = build.build().read_bytes().lower()
    for name in (b"hipblaslt", b"rocblas", b"hipblas"):
        assert name not in blob, f"the library mentions {name!r}"
    needed = subprocess.run(["readelf", "-d", str(build.build())], capture_output=True, text=True).stdout.lower()
    assert "blas" not in needed
    for f in (ROOT / "proxy_inference_engine_amd" / "csrc").iterdir():
        assert not re.search(r"#include\s*<(hipblas|rocblas)", f.read_text(errors="ignore")), f
    lib = _ffi.load()
    assert lib.pie_w16m_bytes(1280, 3420) == 40 * 54 * 4096 and lib.pie_w16m_bytes(0, 64) == 0   # 32-row x 64-column tiles, zero-padded
    assert lib.pie_linear_w16m_workspace(4096, 6144, 4096) == 0                                    # no K split where the tiles fill the chip
    assert lib.pie_linear_w16m_workspace(64, 4096, 14336) % (64 * 4096 * 4) == 0 and lib.pie_linear_w16m_workspace(64, 4096, 14336) > 0


def test_weight_format_entry_points_refuse_before_any_launch_without_gpu():
    """The per-format entry points: every packed size at several (N, K) (0 for odd N, K % 64 != 0 and non-positive sizes), and every
    refusal the repack, streaming-GEMV, quantise / dequantise and embedding functions make before a launch -- its code and the function
    pie_last_error() names.  None of these calls reaches HIP, so they run without a device."""
    from proxy_inference_engine_amd import _ffi
    lib = _ffi.load()
    units = {"pie_w4s_bytes": (2304, 2048), "pie_w8s_bytes": (4352, 2048), "pie_w2s_bytes": (1280, 2048), "pie_w6s_bytes": (3328, 2048),
             "pie_w4s32_bytes": (2560, 2048), "pie_w8s32_bytes": (4608, 2048), "pie_w16s_bytes": (2048, 512)}
    for name, (unit, slice_k) in units.items():
        fn = getattr(lib, name)
        for N, K in ((2, 64), (6, 576), (4096, 4096), (4096, 14336), (1024, 3072), (128256, 4096), (2, 32768), (2, 40960)):
            assert fn(N, K) == (N // 2) * -(-K // slice_k) * unit, (name, N, K)
        for N, K in ((3, 4096), (4, 100), (4, 32), (0, 64), (-2, 64), (2, 0), (2, -64)):
            assert fn(N, K) == 0, (name, N, K)

    buf = ctypes.create_string_buffer(8192)
    base = (ctypes.addressof(buf) + 255) & ~255
    p, odd = ctypes.c_void_p(base), ctypes.c_void_p(base + 2)   # 256-byte aligned / misaligned stand-ins, never dereferenced
    ARG, SHAPE, ALIGN = -1, -2, -3
    BF16, BAD = _ffi.PIE_BF16, 7

    def refused(fn, args, code, who):
        rc = getattr(lib, fn)(*args)
        err = lib.pie_last_error()
        assert rc == code and err.split(b":")[0] == who.encode(), (fn, args, rc, err)

    for fn in ("pie_repack_w4g64", "pie_repack_w8g64", "pie_repack_w2g64", "pie_repack_w6g64", "pie_repack_w4g32", "pie_repack_w8g32"):
        ok = [p, p, p, 8, 256, None, 8, p, None]   # codes, scales, biases, N_src, K, row_map, N_out, packed, stream
        for i, v, code in ((0, None, ARG), (1, None, ARG), (2, None, ARG), (7, None, ARG), (6, 7, SHAPE), (6, 0, SHAPE), (3, 0, SHAPE),
                           (4, 100, SHAPE), (4, 0, SHAPE), (4, 32768 + 64, SHAPE), (7, odd, ALIGN)):
            refused(fn, ok[:i] + [v] + ok[i + 1:], code, fn)
    ok = [p, 8, 256, None, 8, p, None]   # w, N_src, K, row_map, N_out, packed, stream
    for i, v, code in ((0, None, ARG), (5, None, ARG), (4, 7, SHAPE), (1, 0, SHAPE), (2, 100, SHAPE), (2, 32768 + 64, SHAPE), (5, odd, ALIGN),
                       (0, odd, ALIGN)):
        refused("pie_repack_dense", ok[:i] + [v] + ok[i + 1:], code, "pie_repack_dense")

    for fn in ("pie_qgemv_w4g64", "pie_qgemv_w8g64", "pie_qgemv_w2g64", "pie_qgemv_w6g64", "pie_qgemv_w4g32", "pie_qgemv_w8g32", "pie_gemv_dense"):
        for M in (1, 2):   # pie_qgemv_w4g64 takes several rows through the many-row streaming launch
            who = "w4s_gemv_rows" if fn == "pie_qgemv_w4g64" and M > 1 else "w4s_gemv"
            ok = [p, M, p, 64, 256, None, p, BF16, None]   # x, M, packed, N, K, lin_bias, y, dtype, stream
            for i, v, code, by in ((0, None, ARG, fn), (2, None, ARG, fn), (6, None, ARG, fn), (1, 0, SHAPE, fn), (1, 65536, SHAPE, fn),
                                   (0, odd, ALIGN, fn), (2, odd, ALIGN, fn), (4, 100, SHAPE, who), (4, 0, SHAPE, who), (3, 63, SHAPE, who),
                                   (3, 0, SHAPE, who), (4, 32768 + 64, SHAPE, who), (7, BAD, ARG, who)):
                refused(fn, ok[:i] + [v] + ok[i + 1:], code, by)
    ok = [p, 1, p, 64, 256, p, BF16, None]   # x, M, packed, N, K, y (fp32), dtype, stream
    for i, v, code, by in ((0, None, ARG, "pie_qgemv_w4g64_f32"), (5, None, ARG, "pie_qgemv_w4g64_f32"), (1, 0, SHAPE, "pie_qgemv_w4g64_f32"),
                           (4, 100, SHAPE, "w4s_gemv"), (3, 63, SHAPE, "w4s_gemv"), (4, 32768 + 64, SHAPE, "w4s_gemv"), (6, BAD, ARG, "w4s_gemv")):
        refused("pie_qgemv_w4g64_f32", ok[:i] + [v] + ok[i + 1:], code, by)

    ok = [p, 8, 256, 4, BF16, p, p, p, None]   # w, N, K, bits, dtype, codes, scales, biases, stream
    for i, v, code, by in ((0, None, ARG, "pie_quantize_w4g64"), (5, None, ARG, "pie_quantize_w4g64"), (7, None, ARG, "pie_quantize_w4g64"),
                           (3, 3, ARG, "pie_quantize_g64"), (3, 16, ARG, "pie_quantize_g64"), (1, 0, SHAPE, "pie_quantize_w4g64"),
                           (2, 100, SHAPE, "pie_quantize_w4g64"), (0, odd, ALIGN, "pie_quantize_w4g64"), (5, odd, ALIGN, "pie_quantize_w4g64")):
        refused("pie_quantize_g64", ok[:i] + [v] + ok[i + 1:], code, by)
    for bits in (2, 4, 6, 8):
        refused("pie_quantize_g64", ok[:3] + [bits, BAD] + ok[5:], ARG, "pie_quantize_w4g64")
    refused("pie_quantize_w4g64", [None, 8, 256, BF16, p, p, p, None], ARG, "pie_quantize_w4g64")
    refused("pie_quantize_w4g64", [p, 8, 100, BF16, p, p, p, None], SHAPE, "pie_quantize_w4g64")
    refused("pie_quantize_w4g64", [p, 8, 256, BAD, p, p, p, None], ARG, "pie_quantize_w4g64")

    ok = [p, p, p, 8, 256, 4, BF16, p, None]   # codes, scales, biases, N, K, bits, dtype, w_out, stream
    for i, v, code, by in ((0, None, ARG, "pie_dequantize_w4g64"), (7, None, ARG, "pie_dequantize_w4g64"), (5, 2, ARG, "pie_dequantize_g64"),
                           (5, 6, ARG, "pie_dequantize_g64"), (3, 0, SHAPE, "pie_dequantize_w4g64"), (4, 100, SHAPE, "pie_dequantize_w4g64"),
                           (7, odd, ALIGN, "pie_dequantize_w4g64")):
        refused("pie_dequantize_g64", ok[:i] + [v] + ok[i + 1:], code, by)
    for bits in (4, 8):
        refused("pie_dequantize_g64", ok[:5] + [bits, BAD] + ok[7:], ARG, "pie_dequantize_w4g64")
    refused("pie_dequantize_w4g64", [p, p, p, 8, 100, BF16, p, None], SHAPE, "pie_dequantize_w4g64")
    refused("pie_dequantize_w4g64", [p, p, p, 8, 256, BAD, p, None], ARG, "pie_dequantize_w4g64")

    for fn in ("pie_embedding_g64", "pie_embedding_g32"):
        ok = [p, 2, p, p, p, 16, 256, 4, BF16, p, None]   # ids, L, codes, scales, biases, V, H, bits, dtype, out, stream
        for i, v, code, by in ((7, 2, ARG, fn), (7, 6, ARG, fn), (0, None, ARG, "pie_embedding_w4g64"), (2, None, ARG, "pie_embedding_w4g64"),
                               (9, None, ARG, "pie_embedding_w4g64"), (1, 0, SHAPE, "pie_embedding_w4g64"), (5, 0, SHAPE, "pie_embedding_w4g64"),
                               (6, 100, SHAPE, "pie_embedding_w4g64"), (9, odd, ALIGN, "pie_embedding_w4g64")):
            refused(fn, ok[:i] + [v] + ok[i + 1:], code, by)
        for bits in (4, 8):
            refused(fn, ok[:7] + [bits, BAD] + ok[9:], ARG, "pie_embedding_w4g64")
    ok = [p, 2, p, p, p, 16, 256, BF16, p, None]   # ids, L, codes, scales, biases, V, H, dtype, out, stream
    for i, v, code in ((0, None, ARG), (4, None, ARG), (1, 0, SHAPE), (6, 100, SHAPE), (8, odd, ALIGN), (7, BAD, ARG)):
        refused("pie_embedding_w4g64", ok[:i] + [v] + ok[i + 1:], code, "pie_embedding_w4g64")
    ok = [p, 2, p, 16, 256, BF16, p, None]   # ids, L, table, V, H, dtype, out, stream
    for i, v, code in ((0, None, ARG), (2, None, ARG), (6, None, ARG), (1, 0, SHAPE), (4, 100, SHAPE), (5, BAD, ARG), (2, odd, ALIGN),
                       (6, odd, ALIGN)):
        refused("pie_embedding_dense", ok[:i] + [v] + ok[i + 1:], code, "pie_embedding_dense")
