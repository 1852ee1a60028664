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

# Problems that run as K slices over the grid (gemm_ksplit: plain / accumulate epilogue into a dense fp32 C, fewer than 192 tiles of 128
# rows, a long reduction; TN never takes the K-group kernel instead) followed by hamt_reduce_partials -- what they COMPUTE is checked by
# test_gpu_splitk.py, that they split as written here by test_gemm_plan.py.  Rows:
# (switch or None, layout, M, N, K, epilogue, slices of workspace offered or None = as many as hamt_gemm_ksplit asks for, slices, kernel)
def _sk(layout, bm, epi):
    return f"gemm_fast_kernel<{bm}, {EPI_OF[epi]}, {'true' if layout == 'tn' else 'false'}, {'false' if layout == 'nt' else 'true'}>"


def _splitk_rows(switch, bm, rows):
    return [(switch, lay, M, N, K, epi, ws, ks, _sk(lay, bm, epi)) for lay, M, N, K, epi, ws, ks in rows]


EPI_OF = {"none": 0, "bias": 1, "acc": 8, "mulaux": 256, "mulaux8": 256, "gelugrad": 129, "gelugrad8": 129, "drop_res": 1 | 512 | 1024}
SPLITK_GEMMS = _splitk_rows(None, 64, [
    ("tn", 136, 200, 1024, "none", None, 2),       # the smallest problem that splits by itself
    ("tn", 136, 200, 1600, "acc", None, 3),        # 25 k-tiles -> 8, 8, 9
    ("tn", 130, 131, 1600, "none", None, 3),       # N % 4 != 0: element-wise partial store; M N % 4 != 0: the scalar reduce kernel
    ("tn", 64, 128, 2048, "none", None, 4),        # exactly one tile
    ("tn", 200, 300, 8192, "none", None, 16),      # the cap
    ("tn", 200, 300, 8192, "none", 5, 5),          # a smaller workspace than asked for
    ("tn", 200, 300, 8192, "none", 1, 1),          # room for one slice: no split
    ("nt", 100, 1100, 1024, "none", None, 2),
    ("nt", 70, 1030, 1600, "acc", None, 3),        # ragged last column tile, N % 4 != 0
    ("nn", 70, 1032, 1600, "acc", None, 3),
    ("nn", 100, 1100, 1024, "none", None, 2),
    ("nt", 100, 130, 12288, "none", None, 16),     # gemm_kg_variant's "very long reduction" rule (>= 192 k-tiles): not K groups
    ("nn", 100, 136, 12288, "acc", None, 16),
    ("nt", 33, 1, 12288, "none", None, 16),        # one output column
]) + _splitk_rows("HAMT_KS=4", 64, [
    ("nt", 200, 136, 448, "none", None, 4),        # 7 k-tiles -> 1, 2, 2, 2
    ("nn", 200, 136, 448, "acc", None, 4),
    ("tn", 136, 200, 448, "acc", None, 4),
    ("tn", 200, 136, 128, "none", None, 2),        # one k-tile per slice: nothing behind the ring's prologue
    ("nt", 300, 200, 320, "none", None, 4),        # 1, 1, 1, 2
    ("nt", 200, 136, 448, "none", 2, 2),
]) + _splitk_rows("HAMT_FAST_BM=128", 128, [
    ("tn", 136, 200, 1600, "none", None, 3), ("nn", 70, 1032, 1600, "acc", None, 3), ("tn", 130, 131, 1600, "none", None, 3),
]) + _splitk_rows("HAMT_FAST_BM=32", 32, [
    ("nt", 100, 130, 1024, "none", None, 2), ("nn", 100, 136, 1600, "acc", None, 3), ("nt", 33, 1, 1600, "none", None, 3),
])
SPLITK_SWITCHES = ["HAMT_KS=4", "HAMT_FAST_BM=128", "HAMT_FAST_BM=32"]


# ---------------------------------------------------------------------------------------------- hamt_gemm_plan, without a GPU
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLAN_GOLDEN = os.path.join(ROOT, "tests", "golden", "gemm_plan_parent.txt")


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


def splitk_ws_bytes(row, asked):
    """bytes of workspace a SPLITK_GEMMS row offers; `asked` = the slices hamt_gemm_ksplit answers for its descriptor"""
    _, _, M, N, _, _, ws_ks, _, _ = row
    return (asked if ws_ks is None else ws_ks) * M * N * 4


def splitk_mismatches(plan, ksplit, GemmDesc, rows, f32=0):
    """SPLITK_GEMMS rows that `plan(desc, ws_bytes) -> (slices, kernel)` answers differently (`ksplit(desc)`: the slices it asks for)"""
    bad = []
    for r in rows:
        _, layout, M, N, K, epi, _, ks, name = r
        d = plan_desc(GemmDesc, layout, M, N, K, EPI_OF[epi], f32)
        got = plan(d, splitk_ws_bytes(r, ksplit(d)))
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

    if sys.argv[2:] == ["splitk"]:      # the SPLITK_GEMMS rows of this switch instead of the golden record's
        lib.hamt_gemm_ksplit.argtypes = L.SIGNATURES["hamt_gemm_ksplit"]
        mine = [r for r in SPLITK_GEMMS if r[0] == sys.argv[1]]
        bad = splitk_mismatches(_plan, lambda d: lib.hamt_gemm_ksplit(C.byref(d)), L.GemmDesc, mine, L.HAMT_F32)
    else:
        mine = [r for r in plan_golden_rows() if r[0] == sys.argv[1]]
        bad = plan_mismatches(_plan, L.GemmDesc, mine)
    for b in bad[:20]:
        print(b)
    print(f"{sys.argv[1]}: {len(mine)} rows, {len(bad)} mismatches")
    assert "torch" not in sys.modules
    sys.exit(1 if bad or not mine else 0)
