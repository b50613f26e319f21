"""Exact reference, poisoned operands and the case tables of the weight-gradient GEMM seam tests (tests/test_gpu_tn_seams.py; the helper
itself is checked on the host by tests/test_tn_ref_host.py).

    dW[N, K] += dY[M, N]^T . A[M, K]        db[N] += colsum(dY)

Why the comparison needs no tolerance: dY, A and the patch source are integers drawn uniformly from {-3 .. 3}, exact in bf16 and fp32.
Every product has magnitude <= 9, so every partial sum over M <= 8192 rows plus the integer the output starts from stays below 2**24
(max_abs_sum): fp32 accumulation is exact in ANY order -- MFMA, atomics, workspace tree.  Every stored element must equal the fp64
reference bit for bit (torch.equal).  A dropped, doubled or misplaced contraction row changes an element unless the two factors'
product is 0, i.e. with probability 1 - (1 - (6/7)^2) = 36/49 = 73 %.

Every operand lives inside larger poisoned storage (Inputs, Outputs): NaN around what may be read, SENTINEL around what may be written.
Nothing here needs a GPU; `device` decides where the tensors live."""
from dataclasses import dataclass, replace  # noqa: F401  (replace: for the tests that vary a case)
from typing import Optional, Tuple

import torch

INIT = 5.0        # dW / db start here: "accumulates, does not overwrite" is part of every case
SENTINEL = -768.0  # guard value around dW / db (exact in fp32; the guards are compared where they are, never searched for)
NAN = float("nan")
TORCH_DT = {"bf16": torch.bfloat16, "f32": torch.float32}
EPV = {"bf16": 8, "f32": 4}   # elements per 16-byte chunk
BMC = {"bf16": 64, "f32": 32}  # contraction rows per tile of the 128x128 kernel
V1, RING = 1, 2               # lnx_tn_launch.kernel


def roundup(a, b):
    return -(-a // b) * b


# ------------------------------------------------------------------------------------------------------------------------------
# the reference, in plain indexing
# ------------------------------------------------------------------------------------------------------------------------------
def draw(gen, *shape, device="cpu"):
    """integers uniform in {-3 .. 3} as fp32 (generated on the CPU: the same numbers whatever the device)"""
    return torch.randint(-3, 4, shape, generator=gen).to(torch.float32).to(device)


def patch_rows(x):
    """The 2x2 / stride-2 gather: x [B, Hin, Win, Cin] (NHWC) -> A [B Ho Wo, 4 Cin], row m = (b, ho, wo),
    column k = (kh * 2 + kw) * Cin + c  holds  x[b, 2 ho + kh, 2 wo + kw, c]."""
    B, Hin, Win, Cin = x.shape
    Ho, Wo = Hin // 2, Win // 2
    A = x.new_empty(B, Ho, Wo, 4 * Cin)
    for kh in range(2):
        for kw in range(2):
            p = kh * 2 + kw
            A[..., p * Cin:(p + 1) * Cin] = x[:, kh::2, kw::2, :]
    return A.reshape(B * Ho * Wo, 4 * Cin)


def patch_row_of_source(B, Ho, Wo, device="cpu"):
    """[B, 2 Ho, 2 Wo]: the patch row m every source pixel belongs to"""
    m = torch.arange(B * Ho * Wo, device=device).view(B, Ho, Wo)
    return m.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2)


def stored_column(K, k_perm_c):
    """column of dW that contraction column k is stored at: k itself, or with k_perm_c = C > 0 and K = P C: k = p C + c -> c P + p
    (the torch conv weight layout [N, C, kh, kw] for P = 4)"""
    k = torch.arange(K)
    if k_perm_c <= 0:
        return k
    P = K // k_perm_c
    return (k % k_perm_c) * P + k // k_perm_c


def product(dY, A, m_eff):
    """fp64 dY[:m_eff]^T . A[:m_eff] and colsum(dY[:m_eff])"""
    y, a = dY[:m_eff].double(), A[:m_eff].double()
    return y.T @ a, y.sum(0)


def expected_dw(ref, width, k_perm_c=0, k_store=0, init=INIT):
    """what dW[:, :width] holds after the call: init + the product's columns k < k_store (all K when 0) at their stored columns"""
    N, K = ref.shape
    ks = k_store if 0 < k_store < K else K
    col = stored_column(K, k_perm_c)[:ks].to(ref.device)
    out = torch.full((N, width), float(init), dtype=torch.float64, device=ref.device)
    out[:, col] += ref[:, :ks]
    return out


def max_abs_sum(M, init=INIT):
    """bound of every partial sum of a case: 9 M + |init|; below 2**24 every fp32 accumulation order is exact"""
    return 9 * M + abs(init)


# ------------------------------------------------------------------------------------------------------------------------------
# cases
# ------------------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Case:
    dtype: str
    M: int
    N: int
    K: int
    hint: int = 0
    ws: bool = False                 # pass a workspace (sized exactly for the launch, NaN-filled)
    db: bool = True
    lddy: Optional[int] = None       # default roundup(N, chunk) + one chunk
    k_store: int = 0
    lddw: Optional[int] = None       # default: K + 8 guard columns
    k_perm_c: int = 0
    patch: Optional[Tuple[int, int, int, int]] = None  # (B, Ho, Wo, Cin): A is the 2x2 gather from [B, 2 Ho, 2 Wo, Cin]; K = 4 Cin
    m_eff: Optional[int] = None      # m_dev value (None: no m_dev)
    # the path the case is written for (asserted through lnx_gemm_tn_query before the run; None = not pinned)
    kernel: int = RING
    form: Tuple[int, int] = (128, 128)
    splits: Optional[int] = None
    m_per_split: Optional[int] = None
    workspace: bool = False

    @property
    def id(self):
        s = f"{self.dtype}-M{self.M}-N{self.N}-K{self.K}-h{self.hint}"
        if self.patch:
            s += "-patch%dx%dx%dx%d" % self.patch
        if self.k_store:
            s += f"-ks{self.k_store}"
        if self.lddw is not None:
            s += f"-ldw{self.lddw}"
        if self.lddy is not None:
            s += f"-ldy{self.lddy}"
        if self.k_perm_c:
            s += f"-perm{self.k_perm_c}"
        if self.m_eff is not None:
            s += f"-meff{self.m_eff}"
        return s + ("-ws" if self.ws else "-nows") + ("-db" if self.db else "-nodb")


def cdiv(a, b):
    return -(-a // b)


def ring_case(N, K, form, hint=0, M=4096, ws=True, **kw):
    """a bf16 case of the ring kernel; splits / m_per_split as launch_tn's rule gives them for an explicit hint (hint 0: left to the caller)"""
    mt = M // 64
    if hint > 0 and "splits" not in kw:
        per = cdiv(mt, min(hint, mt))
        kw["splits"], kw["m_per_split"] = cdiv(mt, per), per * 64
    return Case("bf16", M, N, K, hint=hint, ws=ws, kernel=RING, form=form, **kw)


WIDE_R, WIDE_C = (256, 128), (128, 256)  # the two tile forms (rows of N x columns of K)
ONE_TILE = {WIDE_R: (256, 128), WIDE_C: (128, 256)}  # (N, K) of one full tile

# Ring length and split seams.  M = 4096 = 64 contraction tiles; hint -> tiles per split: 64 -> 1 (the vmcnt(0) prologue with a single
# issue), 32 -> 2 (no issue inside the loop), 22 -> 3 and a last split of 1, 16 -> 4 (first re-use of stage 0), 13 -> 5 (+4), 10 -> 7 (+1),
# 7 -> 10 (+4), 1 -> 64, 0 -> the automatic rule (8 splits of 8).  The launched split counts 64, 32, 22, 16, 13, 10, 7 exercise the
# second stage's batches of 8: exact batches (64, 32, 16), batches plus remainder (22, 13, 10) and the remainder alone (7).
SPLIT_HINTS = [(64, 64), (32, 32), (22, 22), (16, 16), (13, 13), (10, 10), (7, 7), (1, 1), (0, 8)]
RING_SPLIT_CASES = []
for _form in (WIDE_R, WIDE_C):
    for _hint, _splits in SPLIT_HINTS:
        for _ws in (True, False):
            for _db in (True, False):
                _n, _k = ONE_TILE[_form]
                RING_SPLIT_CASES.append(ring_case(_n, _k, _form, _hint, ws=_ws, db=_db, splits=_splits, m_per_split=cdiv(64, _splits) * 64,
                                                  workspace=_ws and _splits >= 2))
    # 65 contraction tiles, hint 64: 33 splits, two tiles each and ONE in the last
    for _ws in (True, False):
        _n, _k = ONE_TILE[_form]
        RING_SPLIT_CASES.append(ring_case(_n, _k, _form, 64, M=4160, ws=_ws, splits=33, m_per_split=128, workspace=_ws))

# Tile edges, well filled (the workspace path is taken): 2 x 3 tiles of 256x128, 3 x 2 tiles of 128x256, the same with N % 8 != 0 (the
# loader's clamped chunk then reads the NaN padding of dY, which may reach masked rows only); sparse tiles stay on the atomics although a
# workspace is there; k_store / lddw / k_perm_c on both paths.  hint 0 at M = 4096: min(256 / tiles, 8) splits.
RING_EDGE_CASES = [
    ring_case(504, 376, WIDE_R, splits=8, m_per_split=512, workspace=True),
    ring_case(376, 504, WIDE_C, splits=8, m_per_split=512, workspace=True),
    ring_case(500, 376, WIDE_R, lddy=504, splits=8, m_per_split=512, workspace=True),
    ring_case(371, 504, WIDE_C, lddy=376, splits=8, m_per_split=512, workspace=True),
    ring_case(500, 376, WIDE_R, lddy=504, ws=False, splits=8, m_per_split=512),
    ring_case(371, 504, WIDE_C, lddy=376, ws=False, splits=8, m_per_split=512),
    ring_case(264, 136, WIDE_C, splits=8, m_per_split=512, workspace=False),
    ring_case(96, 384, WIDE_C, splits=8, m_per_split=512, workspace=False),
    ring_case(96, 64, WIDE_R, k_store=48, lddw=48, splits=8, m_per_split=512, workspace=False),      # the stem's form (sparse tile: atomics)
    ring_case(96, 64, WIDE_R, k_store=48, lddw=48, hint=3, workspace=False),
    ring_case(256, 128, WIDE_R, k_store=120, lddw=120, splits=8, m_per_split=512, workspace=True),  # k_store in the second stage's mask
    ring_case(256, 128, WIDE_R, k_store=120, lddw=120, ws=False, splits=8, m_per_split=512),        # ... and in the atomics epilogue's
    ring_case(256, 128, WIDE_R, k_perm_c=32, splits=8, m_per_split=512, workspace=True),
    ring_case(256, 128, WIDE_R, k_perm_c=32, ws=False, splits=8, m_per_split=512),
    ring_case(128, 256, WIDE_C, k_perm_c=64, splits=8, m_per_split=512, workspace=True),
    ring_case(128, 256, WIDE_C, k_perm_c=64, ws=False, splits=8, m_per_split=512),
]

# Patch gather on the ring kernel: both forms and the model's own 192 -> 384 downsample, k_perm_c = Cin (conv weight layout), at the
# model's widths (Wo = 7, 14, 28 at 224 input, 12 at 384: qb != 0, the carry fires), non-square, Wo = 64 (qb = 0), Wo > 64 (qa = 0) and
# Wo = 1 (a carry per row).  Each with hint 0 and with a hint whose m_per_split is no multiple of Wo: m_begin inside an image row.
PATCH_FORMS = [(32, 256, WIDE_R), (64, 128, WIDE_C), (192, 384, WIDE_C)]  # (Cin, N, form)
PATCH_GEOMS = [(128, 7, 7), (32, 14, 14), (8, 28, 28), (32, 12, 12), (64, 13, 5), (1, 64, 64), (22, 2, 96), (4096, 1, 1)]


def patch_hint(M, Wo):
    """a split hint with 3 (or 5) contraction tiles per split, so that m_per_split % Wo != 0 where a multiple of 64 allows it at all"""
    per = 3 if (3 * 64) % Wo != 0 or Wo in (1, 64) else 5
    return cdiv(M // 64, per), per * 64


RING_PATCH_CASES = []
for _cin, _n, _form in PATCH_FORMS:
    for _b, _ho, _wo in PATCH_GEOMS:
        _m = _b * _ho * _wo
        _tiles = cdiv(_n, _form[0]) * cdiv(4 * _cin, _form[1])
        _auto = max(1, min(256 // _tiles, (_m // 64) // 8))
        _per = cdiv(_m // 64, _auto)
        RING_PATCH_CASES.append(ring_case(_n, 4 * _cin, _form, M=_m, patch=(_b, _ho, _wo, _cin), k_perm_c=_cin, splits=cdiv(_m // 64, _per),
                                          m_per_split=_per * 64, workspace=True))
        _h, _mps = patch_hint(_m, _wo)
        # (the nine-tile form takes its hinted case through the atomics: 33 splits of nine whole tiles would be a 39 MB workspace)
        _ws = _tiles == 1
        RING_PATCH_CASES.append(ring_case(_n, 4 * _cin, _form, hint=_h, M=_m, patch=(_b, _ho, _wo, _cin), k_perm_c=_cin, ws=_ws, workspace=_ws,
                                          m_per_split=_mps))
# m_dev that is neither a multiple of 64 nor of Wo = 14: a ragged last tile in the middle of an image row
RING_PATCH_CASES += [ring_case(256, 128, WIDE_R, M=6272, patch=(32, 14, 14, 32), k_perm_c=32, m_eff=3001, splits=11, workspace=True),
                     ring_case(128, 256, WIDE_C, hint=33, M=6272, patch=(32, 14, 14, 64), k_perm_c=64, m_eff=3001, ws=False)]

# m_dev at contraction-tile seams: rows at and behind m_eff hold NaN; surplus splits leave zeros in the workspace and nothing in dW.
M_EFFS = lambda M: [0, 1, 63, 64, 65, M - 1, M, M + 7]  # noqa: E731
M_DEV_CASES = []
for _form in (WIDE_R, WIDE_C):
    for _me in M_EFFS(4096):
        for _hint, _splits in ((0, 8), (64, 64)):
            for _ws in (True, False):
                _n, _k = ONE_TILE[_form]
                M_DEV_CASES.append(ring_case(_n, _k, _form, _hint, ws=_ws, m_eff=_me, splits=_splits, workspace=_ws))
for _dt in ("bf16", "f32"):
    for _me in M_EFFS(200):
        for _hint in (0, 64):
            M_DEV_CASES.append(Case(_dt, 200, 128, 128, hint=_hint, m_eff=_me, kernel=V1))

# The 128x128 kernel: bf16 with M < 4096 or M % 64 != 0, fp32 always.
V1_SHAPES = [(5, 8), (128, 128), (129, 136), (200, 264)]  # one tile with a lone chunk, a full tile, one chunk past a tile both ways, 2 x 3 tiles
V1_CASES = []
for _dt in ("bf16", "f32"):
    _b = BMC[_dt]
    for _n, _k in V1_SHAPES:
        for _m in (1, _b - 1, _b, _b + 1, 2 * _b, 3 * _b + 5):
            for _hint in (0, 1):
                V1_CASES.append(Case(_dt, _m, _n, _k, hint=_hint, kernel=V1, splits=1 if _hint == 1 or _m <= 4 * _b else None))
        # a hint larger than the ranges it can fill: 4 -> m_per_split = BMC -> 3 splits, the last of 2 rows
        V1_CASES.append(Case(_dt, 2 * _b + 2, _n, _k, hint=4, kernel=V1, splits=3, m_per_split=_b))
    # the meta-head input layer: K = 16 zero-padded, k_store = lddw = dim
    V1_CASES.append(Case(_dt, 24, 96, 16, k_store=11, lddw=11, kernel=V1, splits=1))
    for _me in (0, 1, _b + 1):
        V1_CASES.append(Case(_dt, 3 * _b + 5, 129, 136, hint=3, m_eff=_me, kernel=V1, splits=2, m_per_split=2 * _b))
# fp32 with the patch gather, the conv weight layout and a k_store below K
for _j in (1, 2, 3):
    V1_CASES.append(Case("f32", 30, 24, 16 * _j, patch=(2, 3, 5, 4 * _j), k_perm_c=4 * _j, k_store=16 * _j - 3, hint=2, kernel=V1, splits=1))
    V1_CASES.append(Case("f32", 30, 24, 16 * _j, patch=(2, 3, 5, 4 * _j), k_perm_c=4 * _j, kernel=V1))
# bf16 at M = 4096 + 32: M % 64 != 0 keeps it off the ring kernel
V1_CASES.append(Case("bf16", 4096 + 32, 128, 128, ws=True, kernel=V1, workspace=False))

# Deferred second stages: one product per tile form and one with the patch gather, each with its own workspace
DEFER_CASES = [ring_case(256, 128, WIDE_R, splits=8, m_per_split=512, workspace=True), ring_case(128, 256, WIDE_C, splits=8, m_per_split=512, workspace=True),
               ring_case(256, 128, WIDE_R, M=4608, patch=(32, 12, 12, 32), k_perm_c=32, splits=9, m_per_split=512, workspace=True)]

ALL_TABLES = {"ring_split": RING_SPLIT_CASES, "ring_edge": RING_EDGE_CASES, "ring_patch": RING_PATCH_CASES, "m_dev": M_DEV_CASES, "v1": V1_CASES,
              "defer": DEFER_CASES}


# ------------------------------------------------------------------------------------------------------------------------------
# the launch decision of a case (lnx_gemm_tn_query: host only)
# ------------------------------------------------------------------------------------------------------------------------------
def lddy_of(c: Case):
    return c.lddy if c.lddy is not None else roundup(c.N, EPV[c.dtype]) + EPV[c.dtype]


def ws_need(q):
    """floats of workspace the ring kernel's launch q needs: a whole 256x128 (or 128x256) tile per split and output tile, then the bias rows"""
    return q.splits * q.tiles_n * q.tiles_k * 256 * 128 + q.splits * q.tiles_n * q.rw


def query_case(c: Case, ws_floats=None):
    """(launch, ws_floats): what lnx_gemm_tn would do with case c and a workspace of ws_floats floats -- by default exactly what the
    launch needs (asked for with an unlimited workspace first), 4096 floats where the 128x128 kernel is given one anyway"""
    from linnaeus_amd import _lib as L
    from linnaeus_amd import ops

    kw = dict(dtype=L.BF16 if c.dtype == "bf16" else L.F32, M=c.M, N=c.N, K=c.K, lddy=lddy_of(c), k_perm_c=c.k_perm_c, k_store=c.k_store, splits=c.hint)
    if c.patch:
        kw["a_patch"] = (2 * c.patch[1], 2 * c.patch[2], c.patch[3])
    else:
        kw["lda"] = c.K + EPV[c.dtype]
    if not c.ws:
        return ops.gemm_tn_query_shape(**kw), 0
    if ws_floats is None:
        q = ops.gemm_tn_query_shape(ws_floats=1 << 40, **kw)
        ws_floats = ws_need(q) if q.kernel == RING else 4096
    return ops.gemm_tn_query_shape(ws_floats=ws_floats, **kw), ws_floats


def assert_path(c: Case, q):
    """the launch q is the path case c was written for"""
    got = dict(kernel=q.kernel, form=(q.rw, q.cw), patch=bool(q.patch), workspace=bool(q.workspace), splits=q.splits, m_per_split=q.m_per_split)
    want = dict(kernel=c.kernel, form=c.form, patch=c.patch is not None, workspace=c.workspace, splits=c.splits if c.splits is not None else q.splits,
                m_per_split=c.m_per_split if c.m_per_split is not None else q.m_per_split)
    assert got == want, f"{c.id}: launched as {got}, the case is written for {want}"


# ------------------------------------------------------------------------------------------------------------------------------
# operands in poisoned storage
# ------------------------------------------------------------------------------------------------------------------------------
EXTRA_ROWS = 3  # NaN rows behind M in dY and A


class Inputs:
    """dY and A (or the patch source) of a case inside NaN storage, and the fp64 product of their first m_eff rows.  Read-only: cached
    and shared between the cases that differ only in how the product is launched or stored."""

    def __init__(self, c: Case, device):
        e = EPV[c.dtype]
        dt = TORCH_DT[c.dtype]
        gen = torch.Generator().manual_seed(1000003 * c.M + 1009 * c.N + c.K + (7 if c.patch else 0))
        M, N, K = c.M, c.N, c.K
        self.m_eff = M if c.m_eff is None else max(0, min(M, c.m_eff))
        self.lddy = lddy_of(c)
        assert self.lddy % e == 0 and self.lddy >= roundup(N, e) and (self.lddy > N or c.lddy is not None)
        dy = draw(gen, M, N, device=device)
        self.dY_store = torch.full((M + EXTRA_ROWS, self.lddy), NAN, dtype=dt, device=device)
        self.dY_store[:self.m_eff, :N] = dy[:self.m_eff]
        self.dY = self.dY_store[:M, :N]
        if c.patch:
            B, Ho, Wo, Cin = c.patch
            assert M == B * Ho * Wo and K == 4 * Cin
            x = draw(gen, B, 2 * Ho, 2 * Wo, Cin, device=device)
            a = patch_rows(x)
            x = x.clone()
            x[patch_row_of_source(B, Ho, Wo, device) >= self.m_eff] = NAN
            self.A_store = torch.full((x.numel() + EXTRA_ROWS * K,), NAN, dtype=dt, device=device)
            self.A_store[:x.numel()] = x.reshape(-1)
            self.A = self.A_store[:x.numel()].view(B, 2 * Ho, 2 * Wo, Cin)
            self.a_patch, self.lda = (2 * Ho, 2 * Wo, Cin), 0
        else:
            self.lda = K + e
            a = draw(gen, M, K, device=device)
            self.A_store = torch.full((M + EXTRA_ROWS, self.lda), NAN, dtype=dt, device=device)
            self.A_store[:self.m_eff, :K] = a[:self.m_eff]
            self.A = self.A_store[:M, :K]
            self.a_patch = None
        self.ref, self.ref_b = product(dy, a, self.m_eff)


class Outputs:
    """dW and db of a case: INIT inside, SENTINEL in the guard columns behind the stored width, in two guard rows behind N and in eight
    guard entries behind db.  An explicit lddw (the stem's and the meta head's k_store = lddw) leaves no guard columns: a store at
    k >= k_store then lands in the next row's first columns (or, from the last row, in the guard rows) and fails the exact comparison."""

    def __init__(self, c: Case, device):
        self.c = c
        ks = c.k_store if 0 < c.k_store < c.K else c.K
        self.width = c.K if c.k_perm_c > 0 else ks
        self.lddw = c.lddw if c.lddw is not None else max(c.K, self.width) + 8
        assert self.lddw >= self.width
        self.dW_store = torch.full((c.N + 2, self.lddw), SENTINEL, dtype=torch.float32, device=device)
        self.dW_store[:c.N, :self.width] = INIT
        self.dW = self.dW_store[:c.N, :self.width]
        self.db_store = torch.full((c.N + 8,), SENTINEL, dtype=torch.float32, device=device)
        self.db_store[:c.N] = INIT
        self.db = self.db_store[:c.N] if c.db else None

    def expected(self, inp: Inputs):
        dw = torch.full_like(self.dW_store, SENTINEL)
        dw[:self.c.N, :self.width] = expected_dw(inp.ref, self.width, self.c.k_perm_c, self.c.k_store).float()
        db = torch.full_like(self.db_store, SENTINEL)
        db[:self.c.N] = (inp.ref_b + INIT).float() if self.c.db else INIT
        return dw, db

    def check(self, inp: Inputs):
        """guards untouched, no NaN in the stored part, every element equal to the fp64 reference bit for bit"""
        c = self.c
        want_w, want_b = self.expected(inp)
        guard_w = torch.ones_like(self.dW_store, dtype=torch.bool)
        guard_w[:c.N, :self.width] = False
        assert bool((self.dW_store[guard_w] == SENTINEL).all()), f"{c.id}: dW guard columns / rows were written"
        assert bool((self.db_store[c.N:] == SENTINEL).all()), f"{c.id}: db guard entries were written"
        assert not bool(torch.isnan(self.dW_store).any()) and not bool(torch.isnan(self.db_store).any()), f"{c.id}: NaN reached dW / db"
        for name, got, want in (("dW", self.dW_store, want_w), ("db", self.db_store, want_b)):
            if not torch.equal(got, want):
                bad = torch.nonzero(got != want)
                first = tuple(bad[0].tolist())
                raise AssertionError(f"{c.id}: {name} differs from the exact reference in {bad.shape[0]} of {got.numel()} elements, the first at {first}: "
                                     f"got {got[first].item()!r}, want {want[first].item()!r}")
