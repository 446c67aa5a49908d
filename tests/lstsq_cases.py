"""The linear-solve matrix: every kernel of csrc/gl_lstsq.hip.h against a float64 normal-equation solve written from the definition
(tests/test_lstsq_solve_host.py checks the matrix and the reference without a GPU, tests/test_gpu_lstsq_solve.py runs it through
gl_lstsq_solve_stack, the solve half of gl_lstsq_fwd on a caller's own stack).

The reference.  LensSimulator.lstsq_simulate solves, per sample,
    W = 1 / err,  X = S W  [HW, D],  Y = obs W,  A = X^T X,  r = X^T Y,  c = pinv(A, rcond = 1e-6, hermitian) r
`reference` is those lines in numpy float64 on the float32 inputs.  No chunks, no tiles, no augmented matrix.

The bound on the normal matrix.  A float32 sum of products in ANY order differs from the exact sum by at most
gamma_m sum_p |X_ip| |X_jp| with gamma_m = m u / (1 - m u), u = 2^-24, when every term passes through at most m roundings (Higham,
Accuracy and Stability of Numerical Algorithms, section 3.1).  m is counted from the code of the kernel that serves the case:
    2 f      the two factors: f = 2 in gl_normal_small_kernel (w = 1 / err is an IEEE division: u; x = s w: u) and f = 3 in the
             MFMA kernels (w by v_rcp_f32, 1 ulp = 2 u; x = s w: u; the multiplication by `keep` in {0, 1} is exact)
  + 1        the rounding of the product x_i x_j
  + chain    additions of the longest chain a lane sees: ceil(chunk / 256) strided pixels in the register kernel; chunk / 4 in the
             MFMA kernels (a wave takes every fourth 16-pixel group of the chunk, 16 pixels = 4 instructions x 4 k-steps each)
  + 6        the wave sum of the register kernel (wave_sum63: six DPP additions); the MFMA accumulators need none
  + 3        the four waves of the workgroup
  + n_chunks - 1   the chunk partials, summed in the solve kernels or by gl_partial_sum_kernel (the same additions)
Nothing in the bound is measured on the kernels."""
import zlib
from dataclasses import dataclass
from typing import Tuple

import numpy as np

U = 2.0 ** -24
RCOND = 1e-6
LS_SMALL, LS_MAXD, LS_LDS_MAXN, LS_MAXN = 8, 80, 127, 255

SMALL = "gl_normal_small_kernel<8>"
PSUM = "gl_partial_sum_kernel"
E2, E4 = "gl_eigh_solve_kernel<2, false>", "gl_eigh_solve_kernel<4, true>"
FAMILIES = ("gl_normal_small_kernel", "gl_normal_mfma_kernel", "gl_normal_pair_kernel", "gl_partial_sum_kernel",
            "gl_chol_solve_kernel", "gl_eigh_solve_kernel")  # (gl_eigh_solve_kernel: two templates' worth, <R, GLOBAL>)


def MFMA(nt, vec):
    return f"gl_normal_mfma_kernel<{nt}, {'true' if vec else 'false'}>"


def PAIR(vec):
    return f"gl_normal_pair_kernel<{'true' if vec else 'false'}>"


def CH(nb):
    return f"gl_chol_solve_kernel<{nb}>"


def short_name(demangled: str) -> str:
    """'void glk::gl_normal_mfma_kernel<3, true>(glk::NormalArgs)' -> 'gl_normal_mfma_kernel<3, true>';
    'glk::gl_partial_sum_kernel(float*, int, int)' -> 'gl_partial_sum_kernel'; '' stays ''"""
    s = demangled.strip()
    if s.startswith("void "):
        s = s[5:]
    if s.startswith("glk::"):
        s = s[5:]
    depth = 0
    for i, ch in enumerate(s):  # cut the parameter list: the first '(' outside the template arguments
        depth += ch == "<"
        depth -= ch == ">"
        if ch == "(" and depth == 0:
            return s[:i]
    return s


# spectrum recipes, one per sample
WELL1, WELL4 = "well_1e1", "well_1e4"
GAP = "gap"            # condition-1e2 body + exact duplicate columns + an all-zero column, all at generic positions (n <= 79)
ZERO_FIRST = "zero_first"  # condition-1e2 body + an all-zero FIRST column (see make_inputs: a certain cut at any n)
EMPTY = "empty"        # the whole sample is zero: coefficients exactly 0
NAN = "nan"            # a well-posed sample with one NaN pixel
RANK_DEFICIENT = (GAP, ZERO_FIRST)
WELL = (WELL1, WELL4)
BOOST = 6.0  # the observation holds this many times each duplicated column of a GAP sample


@dataclass(frozen=True)
class Case:
    id: str
    D: int
    HW: int
    B: int
    want: int            # chunks per sample aimed at: the workgroup target handed to the library is want * B
    chol: bool
    recipes: Tuple[str, ...]  # per sample; a single entry serves every sample
    normal: str          # the three kernels the solve must launch ('' = the stage does not run)
    cholk: str
    eigen: str
    offset: int = 0      # obs / err start this many floats after a 16-byte boundary
    masked: bool = False  # err = +inf on a fifth of the pixels

    @property
    def wgs(self):
        return self.want * self.B

    @property
    def Dp(self):
        return (self.D + 1 + 3) & ~3

    @property
    def chunk(self):
        return chunks(self.HW, self.B, self.wgs)[0]

    @property
    def n_chunks(self):
        return chunks(self.HW, self.B, self.wgs)[1]

    @property
    def kernels(self):
        return (self.normal, self.cholk, self.eigen)

    def recipe(self, b):
        return self.recipes[b if len(self.recipes) > 1 else 0]


def chunks(HW, B, wgs):
    """(pixels per chunk, chunks per sample) as the library lays the normal-matrix launch out"""
    want = max(1, -(-wgs // B))
    per = max(64, -(-(-(-HW // want)) // 64) * 64)
    return per, -(-HW // per)


def C(id, D, HW, B, want, normal, cholk, eigen, recipes=(WELL1,), chol=True, offset=0, masked=False):
    return Case(id, D, HW, B, want, chol, tuple(recipes), normal, cholk, eigen, offset, masked)


CASES = [
    # ---- gl_normal_small_kernel<8>: D + 1 <= 8
    C("small_d1_hw200_one_chunk", 1, 200, 2, 1, SMALL, CH(4), E2),                        # HW < 256 threads, HW < one chunk (256)
    C("small_d3_hw193_masked", 3, 193, 3, 2, SMALL, CH(4), E2, masked=True),               # HW % 64 = 1: a last chunk of one pixel
    C("small_d7_edge_nc9", 7, 576, 1, 9, SMALL, CH(4), E2, recipes=(WELL4,)),              # D + 1 = 8; nine chunks: gl_partial_sum_kernel
    C("small_d5_mixed", 5, 463, 3, 8, SMALL, CH(4), E2, recipes=(WELL1, GAP, EMPTY)),      # HW % 64 = 15, eight chunks
    # ---- gl_normal_mfma_kernel<NT, VEC>: every NT, both VEC, both sides of every tile-row edge
    C("mfma1_d8_edge_vec_nc8", 8, 512, 1, 8, MFMA(1, True), CH(4), E2),                    # D + 1 = 9; HW % 64 = 0; eight chunks
    C("mfma1_d15_edge_hw527", 15, 527, 2, 3, MFMA(1, False), CH(4), E2, recipes=(WELL4, GAP)),   # D + 1 = 16; HW % 64 = 15
    C("mfma2_d16_edge_vec_nc9", 16, 576, 2, 9, MFMA(2, True), CH(4), E2, recipes=(WELL4,)),      # D + 1 = 17; nine chunks
    C("mfma2_d31_edge_offset", 31, 528, 3, 2, MFMA(2, False), CH(4), E2, offset=1),         # D + 1 = 32; HW % 4 = 0, one float off
    C("mfma3_d32_edge_vec_hw528", 32, 528, 2, 4, MFMA(3, True), CH(4), E2, recipes=(WELL1, GAP)),  # D + 1 = 33; HW % 64 = 16
    C("mfma3_d47_edge_hw593", 47, 593, 1, 5, MFMA(3, False), CH(4), E2, recipes=(WELL4,)),  # D + 1 = 48; HW % 64 = 17
    C("mfma4_d48_edge_vec_masked", 48, 640, 2, 3, MFMA(4, True), CH(4), E2, masked=True),   # D + 1 = 49
    C("mfma4_d63_edge_chol4", 63, 705, 2, 4, MFMA(4, False), CH(4), E2, recipes=(WELL4, GAP)),   # D + 1 = 64; WaveCtxN<2> n = 63
    C("mfma5_d64_edge_chol5_vec", 64, 704, 2, 1, MFMA(5, True), CH(5), E2, recipes=(WELL4, GAP)),  # D + 1 = 65; n = 64; one chunk
    C("mfma5_d65_hw831", 65, 831, 2, 6, MFMA(5, False), CH(5), E2, recipes=(WELL1, GAP)),   # n = 65: the split ballot's second register
    C("mfma5_d79_edge_vec_nan", 79, 768, 3, 2, MFMA(5, True), CH(5), E2, recipes=(WELL1, NAN, WELL4)),  # D + 1 = 80 (LS_MAXD)
    C("mfma2_d20_b33", 20, 320, 33, 2, MFMA(2, True), CH(4), E2, recipes=(WELL1,) * 14 + (GAP,) * 3 + (WELL4,) * 15 + (EMPTY,)),
    C("mfma3_d40_chol_off", 40, 449, 2, 8, MFMA(3, False), "", E2, recipes=(WELL4, GAP), chol=False),  # HW % 64 = 1
    # ---- gl_normal_pair_kernel<VEC>: D + 1 > 80; 2, 3 and 4 super-blocks
    C("pair_d80_edge_chol8_vec", 80, 832, 2, 2, PAIR(True), CH(8), E2, recipes=(WELL4, ZERO_FIRST)),    # D + 1 = 81
    C("pair_d127_edge_lds", 127, 1217, 2, 3, PAIR(False), CH(8), E2, recipes=(WELL4, ZERO_FIRST)),       # D = 127, D + 1 = 128; n = 127
    C("pair_d128_edge_global_vec", 128, 1152, 2, 9, PAIR(True), "", E4, recipes=(WELL4, ZERO_FIRST)),    # D = 128, D + 1 = 129; n = 128
    C("pair_d129_offset", 129, 1280, 2, 2, PAIR(False), "", E4, recipes=(WELL1, ZERO_FIRST), offset=1),  # n = 129
    C("pair_d100_masked_nc8", 100, 1024, 1, 8, PAIR(True), CH(8), E2, recipes=(WELL4,), masked=True),
    C("pair_d191_edge", 191, 1551, 1, 4, PAIR(False), "", E4, recipes=(WELL4,)),             # D + 1 = 192: three super-blocks
    C("pair_d192_edge_vec", 192, 1600, 2, 3, PAIR(True), "", E4, recipes=(WELL1, ZERO_FIRST)),  # D + 1 = 193: four; n = 192
    C("pair_d193", 193, 1617, 2, 5, PAIR(False), "", E4, recipes=(WELL4, ZERO_FIRST)),        # n = 193; HW % 64 = 17
    C("pair_d255_edge_vec", 255, 2048, 2, 4, PAIR(True), "", E4, recipes=(WELL1, ZERO_FIRST)),  # D = 255: the last size served
    C("pair_d120_chol_off", 120, 1100, 1, 1, PAIR(True), "", E2, recipes=(WELL4,), chol=False),  # LDS eigen solve at 120 without attempt
]


def declared_names():
    """every kernel name the matrix claims to launch (gl_partial_sum_kernel where a case has more than eight chunks)"""
    names = {k for c in CASES for k in c.kernels if k}
    if any(c.n_chunks > 8 for c in CASES):
        names.add(PSUM)
    return names


# ---- inputs -----------------------------------------------------------------------------------------------------------------
def _rng(case, salt):
    return np.random.default_rng(zlib.crc32(f"{case.id}/{salt}".encode()))


def gap_layout(case, b):
    """(duplicates [(copy, original)], zero columns) of a rank-deficient sample"""
    D, recipe = case.D, case.recipe(b)
    if recipe == ZERO_FIRST:
        return [], [0]
    if recipe != GAP:
        return [], []
    r = _rng(case, f"gap{b}")
    k = 1 if D < 8 else 2
    cols = r.permutation(D)  # generic positions: the active block of the eigen solve spans all n entries
    return [(int(cols[2 * i]), int(cols[2 * i + 1])) for i in range(k)], [int(cols[2 * k])]


def null_vectors(case, b):
    """Unit vectors of the null space of a rank-deficient sample's normal matrix: e_z per zero column, (e_d - e_o) / sqrt(2) per
    duplicate pair.  The minimum-norm solution is orthogonal to each."""
    dups, zeros = gap_layout(case, b)
    out = []
    for z in zeros:
        v = np.zeros(case.D)
        v[z] = 1.0
        out.append(v)
    for d, o in dups:
        v = np.zeros(case.D)
        v[d], v[o] = np.sqrt(0.5), -np.sqrt(0.5)
        out.append(v)
    return out


def null_bound(w):
    """|n . c| <= u (lambda_max / lambda_min) max |c| for a unit null vector n of the normal matrix, lambda over the KEPT float64
    eigenvalues `w` of the sample.  First-order perturbation theory: a float32 eigen solve returns the exact vectors of A + E with
    |n^T E v_k| of the order u lambda_max, which tilts each kept vector v_k by u lambda_max / lambda_k towards n; the solution
    sum_k v_k g_k then picks up sum_k (u lambda_max / lambda_k) g_k along n, the terms of mixed sign and largest where lambda_k is
    smallest.  This is what 'a coefficient at rounding level' means for a body of a given condition: 1.8e-7 max |c| at the
    condition 3 of test_eigh_host's rank-deficient system (which asserts 1e-6 there), 6e-6 max |c| at condition 1e2."""
    kept = w[np.abs(w) > RCOND * np.abs(w).max()]
    return U * kept.max() / kept.min()


def mask_of(case):
    """True = masked (err = +inf): every fifth pixel, from a case-dependent phase"""
    m = np.zeros(case.HW, dtype=bool)
    if case.masked:
        m[zlib.crc32(case.id.encode()) % 5::5] = True
    return m


def _design(r, rows, n, cond):
    """[rows, n] with singular values geomspace(1, 1 / sqrt(cond)) x 37 from orthonormal factors (float64)"""
    Uo, _ = np.linalg.qr(r.normal(size=(rows, n)))
    Wo, _ = np.linalg.qr(r.normal(size=(n, n)))
    return (Uo * np.geomspace(1.0, 1.0 / np.sqrt(cond), n)) @ Wo.T * 37.0


def make_inputs(case, nan=True):
    """(stack [B, D, HW], obs [HW], err [HW]) in float32.  The weighted design X = S / err of a sample is built in float64 from
    orthonormal factors on the unmasked pixels; S = float32(X err).  Duplicates are bitwise copies of a float32 column, zero
    columns are exact zeros; with `nan=False` the NaN pixel of a NAN sample keeps its finite value.

    GAP puts its duplicates and its zero column at generic positions, so the QL iteration works on all n entries; the host twin
    confirms at these sizes (n <= 79) that float32 makes numpy's cut.  The observation carries BOOST times every duplicated
    column, so the shared amplitude of a pair is comparable to max |c| and can be held to a fraction of itself.
    ZERO_FIRST serves the sizes beyond: float32 eigenvalue noise around a generic zero eigenvalue grows with n and reaches the
    cutoff 1e-6 lambda_max = 16.8 u lambda_max at n in the hundreds, where the cut would be a coin toss.  Row and column 0 of the
    normal matrix are exactly zero in any arithmetic; every reflector of the Householder reduction has v[0] = A[i][0] = 0 and
    leaves them so; the tridiagonal comes out with d[0] = e[1] = 0: an exact zero eigenvalue, cut for certain, and the QL
    iteration runs on entries 1 .. n - 1, which keep their lane positions (every register of the wave context up to index n - 1
    holds live entries; the ballots cross 63 / 64, 127 / 128, 191 / 192 at the listed n).  The coefficient of that zero column
    is exactly 0 by construction, so the null-direction check is vacuous for ZERO_FIRST samples: the GAP samples carry it."""
    B, D, HW = case.B, case.D, case.HW
    r = _rng(case, "inputs")
    live = ~mask_of(case)
    rows = int(live.sum())
    err = r.uniform(0.5, 2.0, size=HW).astype(np.float32)
    stack = np.zeros((B, D, HW), dtype=np.float32)
    y, boost = np.zeros(HW), np.zeros(HW)
    for b in range(B):
        recipe = case.recipe(b)
        if recipe == EMPTY:
            continue
        dups, zeros = gap_layout(case, b)
        free = [c for c in range(D) if c not in zeros and c not in [d for d, _ in dups]]
        cond = {WELL1: 1e1, WELL4: 1e4, NAN: 1e1}.get(recipe, 1e2)
        X = _design(r, rows, len(free), cond)
        S = np.zeros((D, HW), dtype=np.float32)
        S[np.ix_(free, np.flatnonzero(live))] = (X * err[live].astype(np.float64)[:, None]).T.astype(np.float32)
        S[:, ~live] = r.normal(size=(D, int((~live).sum()))).astype(np.float32) * np.float32(9.0)  # masked pixels carry anything
        for zc in zeros:
            S[zc] = 0
        for d, o in dups:
            S[d] = S[o]
        if b == 0:  # one observation for the batch: sample 0's model plus noise
            y[live] = X @ r.normal(size=len(free)) + 0.3 * r.normal(size=rows)
        for _, o in dups:
            boost[live] += BOOST * X[:, free.index(o)]
        if recipe == NAN and nan:
            S[D // 2, HW // 2] = np.nan  # between two finite samples
        stack[b] = S
    if not y.any():
        y[live] = r.normal(size=rows)
    obs = ((y + boost) * err).astype(np.float32)
    obs[~live] = np.float32(5.0)
    err[~live] = np.inf
    return stack, obs, err


# ---- the float64 reference, from the definition -----------------------------------------------------------------------------
def weighted(stack_b, obs, err, drop_masked=True):
    """X [HW', D], Y [HW'] in float64; masked pixels are REMOVED (not weighted by zero) when drop_masked"""
    keep = np.isfinite(err) if drop_masked else np.ones(err.shape, dtype=bool)
    W = 1.0 / err[keep].astype(np.float64)
    return (stack_b[:, keep].astype(np.float64) * W).T, obs[keep].astype(np.float64) * W


def reference(stack_b, obs, err):
    """(A, r, c) of one sample: W = 1 / err, X = S W, Y = obs W, A = X^T X, r = X^T Y, c = pinv(A, 1e-6, hermitian) r"""
    X, Y = weighted(stack_b, obs, err)
    A = X.T @ X
    r = X.T @ Y
    return A, r, np.linalg.pinv(A, rcond=RCOND, hermitian=True) @ r


def augmented_reference(stack_b, obs, err):
    """(M, |M|): the augmented normal matrix [X | Y]^T [X | Y], [D + 1, D + 1], and the same sum over absolute products"""
    X, Y = weighted(stack_b, obs, err)
    Z = np.concatenate([X, Y[:, None]], axis=1)
    return Z.T @ Z, np.abs(Z).T @ np.abs(Z)


# ---- the derived bound ------------------------------------------------------------------------------------------------------
def gamma(m):
    return m * U / (1.0 - m * U)


def rounding_count(case, kernel=None):
    """m of the module docstring for the normal-matrix kernel that serves `case` (default: the declared one)"""
    name = kernel or case.normal
    if name == SMALL:
        return 2 * 2 + 1 + -(-case.chunk // 256) + 6 + 3 + (case.n_chunks - 1)
    return 2 * 3 + 1 + case.chunk // 4 + 3 + (case.n_chunks - 1)


def normal_bound(case, absM):
    return gamma(rounding_count(case)) * absM
