"""GEMM problems whose kernel choice is pinned: asserted after real launches by test_gpu_ops.py and, without a GPU, on hamt_gemm_plan by
test_gemm_plan.py."""
import ctypes as C
import os
import sys

# (layout, (M, N, K), prefix of the kernel name): small grids with a long reduction run as K groups inside one workgroup
KG_GEMMS = [
    ("nt", (1280, 768, 3072), "gemm_kg_kernel<32, 2, 4"), ("nn", (1280, 768, 2304), "gemm_kg_kernel<32, 2, 4"),
    ("nt", (1968, 768, 3072), "gemm_kg_kernel<64, 3, 2"), ("nn", (1968, 768, 2304), "gemm_kg_kernel<64, 3, 2"),
    ("nt", (688, 768, 768), "gemm_kg_kernel<32, 2, 4"), ("nt", (100, 130, 1536), "gemm_kg_kernel<32, 2, 4"),
    ("nn", (1301, 700, 1600), "gemm_kg_kernel<32, 2, 4"), ("nn", (2500, 520, 1664), "gemm_kg_kernel<64, 3, 2"),
    ("nt", (5120, 768, 3072), "gemm_kg_kernel<128, 2, 2"), ("nn", (2752, 768, 2304), "gemm_kg_kernel<128, 2, 2"),
    ("nn", (4001, 1000, 2368), "gemm_kg_kernel<128, 2, 2")]

# The step's own GEMM shapes at the benchmarked per-GPU batch (B = 64: text 5120 rows, panorama 11520, text + vision 7872 ...),
# each on the kernel the launcher picks for it there, against fp64 products of the same bf16-rounded operands.  The smaller
# SHAPES above never reach the 256-square two-phase tile (gemm_p8_kernel needs >= ~200 tiles and K >= 128) nor the 128-row plain
# tile; round 2 shipped a NaN in exactly that family which only a training soak saw.
BENCH_GEMMS = [   # (layout, M, N, K, epilogue, C dtype, kernel the launcher must pick)
    ("nt", 5120, 2304, 768, "bias", "bf16", "gemm_p8_kernel<1, false, false, 3>"),       # text QKV: 240 tiles of 256 x 192 = one full round
    ("nt", 7872, 2304, 768, "bias", "bf16", "gemm_fast_kernel<128, 1, false, false>"),   # packed QKV over text + vision rows: two rounds of either 256-row tile -> plain 128-row tiles
    ("nt", 11520, 2304, 768, "bias", "bf16", "gemm_p8_kernel<1, false, false, 4>"),         # panorama QKV
    ("nt", 5120, 3072, 768, "gelugrad", "bf16", "gemm_p8_kernel<129, false, false, 4>"),    # text FFN-1 (+ saved gelu')
    ("nt", 11520, 3072, 768, "gelugrad", "bf16", "gemm_p8_kernel<129, false, false, 4>"),   # panorama FFN-1
    ("nt", 5003, 2304, 768, "bias", "bf16", "gemm_p8_kernel<1, false, false, 3>"),       # ragged last tile row
    ("nt", 5120, 2304, 768, "gelugrad", "bf16", "gemm_p8_kernel<129, false, false, 3>"), # (FFN-1's epilogue on the narrow tile)
    ("nt", 5120, 2250, 768, "bias", "f32", "gemm_p8_kernel<1, false, false, 3>"),        # ragged last 192-column tile (138 columns), fp32 C
    ("nt", 5120, 2318, 768, "bias", "f32", "gemm_p8_kernel<1, false, false, 4>"),           # ragged last tile column, fp32 C
    ("nt", 11520, 768, 3072, "bias", "bf16", "gemm_p8_kernel<1, false, false, 3>"),      # panorama FFN-2
    ("nt", 11520, 768, 3072, "drop_res", "f32", "gemm_p8_kernel<1537, false, false, 4>"),   # bias + dropout + residual (pre-LN ViT form)
    ("nn", 5120, 3072, 768, "mulaux", "bf16", "gemm_p8_kernel<256, false, true, 4>"),       # dgrad of FFN-2 x gelu'
    ("nn", 11520, 3072, 768, "mulaux", "bf16", "gemm_p8_kernel<256, false, true, 3>"),
    ("nn", 11520, 768, 3072, "acc", "f32", "gemm_p8_kernel<8, false, true, 3>"),         # dgrad of FFN-1 into the residual gradient
    ("nn", 11520, 768, 2304, "acc", "f32", "gemm_p8_kernel<8, false, true, 3>"),         # dgrad of QKV into the residual gradient
    ("nn", 5120, 2304, 768, "none", "bf16", "gemm_p8_kernel<0, false, true, 3>"),
    ("nn", 5013, 2248, 768, "mulaux", "bf16", "gemm_p8_kernel<256, false, true, 3>"),    # ragged rows and a ragged 192-column tile, K-strided B
    ("nn", 5009, 3072, 768, "mulaux", "bf16", "gemm_p8_kernel<256, false, true, 4>"),       # ragged rows
    ("nt", 5120, 768, 768, "bias", "bf16", "gemm_q4_kernel<1, false>"),                  # attention output projection: 240 tiles of 128 x 128, four-deep ring
    ("nn", 5120, 768, 768, "none", "bf16", "gemm_q4_kernel<0, true>"),                   # its dgrad
    ("nt", 2752, 768, 768, "bias", "f32", "gemm_q4_kernel<1, false>"),                   # vision stream (132 tiles)
    ("nt", 1280, 768, 768, "bias", "bf16", "gemm_kg_kernel<32, 2, 4, false>"),           # (B = 16: too few 128-square tiles -- K groups on 32-row tiles)
    ("nn", 1280, 768, 768, "none", "bf16", "gemm_kg_kernel<32, 2, 4, true>"),
    ("nt", 5120, 1536, 768, "bias", "bf16", "gemm_fast_kernel<128, 1, false, false>"),   # key / value projection of the cross attention (N = 1536: not the q4 tile's)
    ("nt", 5003, 760, 832, "bias", "f32", "gemm_q4_kernel<1, false>"),                   # ragged rows and columns
    ("nn", 5003, 760, 832, "acc", "f32", "gemm_q4_kernel<8, true>"),
    ("nn", 5120, 768, 2304, "acc", "f32", "gemm_q4_kernel<8, true>"),                    # dgrad of QKV into the residual gradient
    ("nt", 3200, 768, 192, "bias", "bf16", "gemm_q4_kernel<1, false>"),                  # the shortest reduction the ring takes (3 k-tiles)
    ("nt", 3200, 768, 256, "none", "bf16", "gemm_q4_kernel<0, false>"),
    ("nt", 4096, 4096, 64, "bias", "bf16", "gemm_fast_kernel<128, 1, false, false>"),    # 128-row plain tile
    ("nn", 4096, 4096, 64, "acc", "f32", "gemm_fast_kernel<128, 8, false, true>"),
    ("nt", 5120, 3072, 768, "gelugrad8", "bf16", "gemm_p8_kernel<129, false, false, 4>"),   # text FFN-1, gelu' saved as one byte (HAMT_U8G)
    ("nt", 2752, 3072, 768, "gelugrad8", "bf16", None),                                      # vision stream
    ("nt", 389, 3068, 768, "gelugrad8", "bf16", None),                                       # ragged rows / columns: byte-wise tail of the code image
    ("nn", 5120, 3072, 768, "mulaux8", "bf16", "gemm_p8_kernel<256, false, true, 4>"),       # dgrad of FFN-2 x the one-byte gelu'
    ("nn", 11520, 3072, 768, "mulaux8", "bf16", "gemm_p8_kernel<256, false, true, 3>"),
    ("nn", 2752, 3072, 768, "mulaux8", "bf16", None),
    ("nn", 389, 3068, 768, "mulaux8", "bf16", None),
    ("nt", 5120, 768, 3072, "bias", "bf16", "gemm_q4_kernel<1, false>"),                  # text FFN-2
    ("nn", 5120, 768, 3072, "acc", "f32", "gemm_q4_kernel<8, true>"),
]


# ---------------------------------------------------------------------------------------------- hamt_gemm_plan, without a GPU
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLAN_GOLDEN = os.path.join(ROOT, "tests", "golden", "gemm_plan_parent.txt")
EPI_OF = {"none": 0, "bias": 1, "acc": 8, "mulaux": 256, "mulaux8": 256, "gelugrad": 129, "gelugrad8": 129, "drop_res": 1 | 512 | 1024}


def plan_desc(GemmDesc, layout, M, N, K, epilogue, dtype_c):
    """The descriptor ops.gemm builds for bf16 operands stored densely (K-strided operands: rows padded to 16 bytes), C and aux N wide."""
    a_km, b_km = int(layout == "tn"), int(layout != "nt")
    r8 = lambda x: (x + 7) // 8 * 8
    d = GemmDesc(M, N, K, r8(M) if a_km else K, r8(N) if b_km else K, N, N, a_km, b_km, 1, 1, dtype_c, 0, 0, epilogue, 1.0, 0, 0, 0.0, 0, None)
    if epilogue & 1024:
        d.p_drop, d.rng = 0.1, 0x1000       # (never read: nothing is launched)
    return d


def plan_golden_rows():
    """(environment, layout, M, N, K, epilogue, dtype_c, slices the workspace is sized for, slices, kernel) of tests/golden/gemm_plan_parent.txt"""
    rows, env = [], None
    for line in open(PLAN_GOLDEN):
        if line.startswith("["):        # "[environment]" heads that setting's rows
            env = line.strip()[1:-1]
        elif line.strip() and not line.startswith("#"):
            f = line.rstrip("\n").split("\t")
            rows.append((env, f[0]) + tuple(int(x) for x in f[1:8]) + (f[8],))
    return rows


def plan_mismatches(plan, GemmDesc, rows):
    """rows that `plan(desc, ws_bytes) -> (slices, kernel)` answers differently"""
    bad = []
    for r in rows:
        _, layout, M, N, K, e, dc, ws_ks, ks, name = r
        got = plan(plan_desc(GemmDesc, layout, M, N, K, e, dc), ws_ks * M * N * 4 if ws_ks > 1 else 0)
        if got != (ks, name):
            bad.append((r, got))
    return bad


if __name__ == "__main__":      # child of test_gemm_plan.py: the rows of ONE environment setting (already in os.environ), no torch in the process
    sys.path.insert(0, ROOT)
    from vln_hamt_amd import _lib as L
    lib = C.CDLL(L.LIB_PATH)
    lib.hamt_gemm_plan.argtypes = L.SIGNATURES["hamt_gemm_plan"]
    buf = C.create_string_buffer(160)

    def _plan(d, ws_bytes):
        ks = lib.hamt_gemm_plan(C.byref(d), ws_bytes, buf, 160)
        return ks, buf.value.decode()

    mine = [r for r in plan_golden_rows() if r[0] == sys.argv[1]]
    bad = plan_mismatches(_plan, L.GemmDesc, mine)
    for b in bad[:20]:
        print(b)
    print(f"{sys.argv[1]}: {len(mine)} rows, {len(bad)} mismatches")
    assert "torch" not in sys.modules
    sys.exit(1 if bad or not mine else 0)
