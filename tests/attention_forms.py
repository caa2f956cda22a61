"""The contract of the attention entry points (include/msclip_hip.h: msclip_attention, _varlen, _lastq, _lastq_varlen, _bwd,
_bwd_varlen) as a checker, per element:

    S = q k^T (+ causal mask), P = softmax(S), O = P v                              per (sample, head), head_dim 64, q pre-scaled
    dV = P^T dO, dP = dO v^T, delta = sum_k P dP, dS = P (dP - delta), dQ = dS k, dK = dS^T q
    stored: the live rows, columns [0, heads*64) of out and [0, 3*heads*64) of dqkv; the pad rows behind cu[nsamples] of the
    packed forms as zeros; one row per sample for the single-query forms -- and nothing else.  Read: the live rows' q | k | v
    (k | v for the single-query forms) and dout columns, nothing else (`o` of the backward not at all).

reference() states that in fp64, bound() is a per-element error bound derived from the kernels' documented rounding points (not
from their output), worst() the largest |got - expected| / bound over the stored elements (inf when anything else moved, nan
when a stored element is NaN), per third of dqkv.  A case passes with worst <= MARGIN.

MARGIN.  emulate() applies the kernels' rounding points to the fp64 statement (bf16 P and dS operands, fp32 row sum and delta,
bf16 stores).  Over every case of the sweep of tests/test_gpu_attention_forms.py (all L values and length lists below, 5 heads,
both masks, the four value regimes, run on the CPU) its largest ratio is EMULATION_MAX = 1.10 for O (0.86 for the single-query
forms) and 1.83 for dqkv; MARGIN = 2 * EMULATION_MAX = 2.2 / 3.66, the factor 2 for what the emulation does not model (the accumulation order, __expf / v_exp against exp).  MARGIN is never tuned from the
GPU's output: a kernel beyond it is a rounding point the model lacks (documented and added to bound()) or a defect.

tests/test_attention_forms_cpu.py shows what the checker can see; tests/test_gpu_attention_forms.py runs every kernel
instantiation.  No fixtures, no hooks: an ordinary module."""
import math
from collections import namedtuple
from types import SimpleNamespace

import torch

BF = torch.bfloat16
HD = 64
U = 2.0 ** -9                      # unit roundoff of bf16 round-to-nearest-even (f32_to_bf16 / pack_bf16x2, csrc/common.h)
EPS32 = 2.0 ** -24                 # fp32
N_ACC = 288 * EPS32                # an fp32 sum of at most 288 terms (the longest key / query axis)
E_DOT = 8 * EPS32                  # a 64-term fp32 dot product of exact bf16 products: sqrt(64) roundings (see bound())
E_EXP = 2.0 ** -21                 # __expf / v_exp_f32: relative error of order 2^-21 (1 + |argument|)
TINY = 2.0 ** -125                 # twice the smallest normal fp32 / bf16 value: below it a value may be flushed to zero (see bound())

# Largest worst() of emulate() over the sweep's cases (measured on the CPU, see the module docstring) and the pass mark.
EMULATION_MAX = {"fwd": 1.10, "bwd": 1.83}
MARGIN = {k: 2.0 * v for k, v in EMULATION_MAX.items()}

# ---- the sweep's axes (shared by the GPU sweep and the MARGIN measurement) ---------------------------------------------------
FWD_L = (1, 32, 33, 64, 65, 96, 97, 197, 224, 225, 257, 288)
FWD_WAVE_L = (97, 197, 224)
LASTQ_L = (1, 32, 33, 64, 65, 80, 81, 128, 129, 256, 257, 288)
BWD_L = (1, 33, 64, 65, 96, 97, 160, 161, 208, 209, 257, 272)
PACKED = ((1, 32, 7, 2), (33, 1, 64, 20), (96, 2, 65, 1, 31))            # Lmax 32, 64, 96
LASTQ_PACKED = ((32, 1, 9), (33, 64, 2), (65, 3, 80), (81, 96, 5))          # one list per single-query width up to 96
REGIMES = ("plain", "sharp", "offset", "wide")
K_OFFSET, V_OFFSET = 2.0, 3.0

# One operand layout.  pad: leading dimension - width; col0: first column of the window; base / tail: rows of the buffer in
# front of / behind the block.  Every offset is a multiple of 8 elements (16-byte row pieces stay aligned).
Layout = namedtuple("Layout", "name pad col0 base tail")
TIGHT = Layout("tight", 0, 0, 0, 3)
WINDOW = Layout("window", 64, 24, 5, 3)
LAYOUTS = (TIGHT, WINDOW)
GUARD = 32                         # further rows behind `tail` in every buffer: a kernel that took the wrong branch (a longer tile count,
                                   # an unclamped row) computes a wrong number or moves a guarded bit, never an address outside an allocation


class Rows:
    """Row layout of the samples inside the block: fixed (sample b = rows b*L ..) or packed (rows cu[b] .. cu[b + 1], then
    pad_rows rows of tile padding)."""

    def __init__(self, lens, packed, pad_rows=0):
        self.lens, self.packed, self.pad_rows = list(lens), packed, pad_rows
        self.n, self.L = len(self.lens), max(self.lens)
        self.starts = [sum(self.lens[:b]) for b in range(self.n)]
        self.live = sum(self.lens)
        self.block = self.live + pad_rows

    @classmethod
    def fixed(cls, L, nsamples):
        return cls([L] * nsamples, False)

    def cu(self, device):
        return torch.tensor(self.starts + [self.live, self.L], dtype=torch.int32, device=device)


# ---- data ------------------------------------------------------------------------------------------------------------------
def make_data(rows, heads, regime, seed, device="cpu", nq=None):
    """bf16 q | k | v rows [live, 3*heads*64] and dout rows [live, heads*64] (and, nq: the compact query rows [nq, heads*64]
    of the single-query forms) in one of the four value regimes."""
    g = torch.Generator().manual_seed(seed)
    W = heads * HD
    q, k, v, do = (0.7 * torch.randn(rows.live, W, generator=g) for _ in range(4))
    qc = 0.7 * torch.randn(nq or 1, W, generator=g)
    scale = {"plain": 1.0, "sharp": 6.0, "offset": 1.0, "wide": 14.0}[regime]
    if regime == "offset":
        k, v = k + K_OFFSET, v + V_OFFSET
    d = SimpleNamespace(qkv=torch.cat([q * scale, k, v], 1).to(BF).to(device), dout=(do / 0.7).to(BF).to(device),
                        qc=(qc * scale).to(BF).to(device))
    return d


class Buffers:
    """The buffers of one call.  Inputs: NaN (bf16 0x7fc0) everywhere the contract does not let the call read -- the rows in
    front of the block and behind its last live row (pad rows included), the gap columns of a window, the q columns of the
    token matrix for the single-query forms, the whole `o` -- and the data elsewhere.  Outputs: a finite random pattern, so
    that "changed a bit" is decidable.  front: further rows in front of the token matrix (row_base of the single-query forms)."""

    def __init__(self, data, rows, heads, layout, device, seed, front=0, single=False):
        W, lay = heads * HD, layout
        self.lay, self.rows, self.heads, self.front = lay, rows, heads, front
        nrows = front + lay.base + rows.block + lay.tail + GUARD
        self.ldq, self.ldo = 3 * W + lay.pad, W + lay.pad
        nan = float("nan")
        self.qkv = torch.full((nrows, self.ldq), nan, dtype=BF, device=device)
        r0 = front + lay.base
        c0 = W if single else 0
        self.qkv[r0:r0 + rows.live, lay.col0 + c0:lay.col0 + 3 * W] = data.qkv[:, c0:]
        g = torch.Generator().manual_seed(seed)
        rnd = lambda r, c, dt: (torch.randn(r, c, generator=g) * 0.37).to(dt).to(device)
        if single:
            n = rows.n
            self.qc = torch.full((lay.base + n + lay.tail + GUARD, self.ldo), nan, dtype=BF, device=device)
            self.qc[lay.base:lay.base + n, lay.col0:lay.col0 + W] = data.qc
            self.out = rnd(lay.base + n + lay.tail + GUARD, self.ldo, BF)
        else:
            self.dout = torch.full((lay.base + rows.block + lay.tail + GUARD, self.ldo), nan, dtype=BF, device=device)
            self.dout[lay.base:lay.base + rows.live, lay.col0:lay.col0 + W] = data.dout
            self.o = torch.full_like(self.dout, nan)
            self.out = rnd(lay.base + rows.block + lay.tail + GUARD, self.ldo, BF)
            self.dqkv = rnd(lay.base + rows.block + lay.tail + GUARD, self.ldq, BF)
            self.part = rnd(rows.n + 1, 3 * W, torch.float32)
        self.out0 = self.out.clone()
        if not single:
            self.dqkv0, self.part0 = self.dqkv.clone(), self.part.clone()

    def view(self, t, front=0):
        """The block as the call sees it: row 0 = the first row behind base (and front), column 0 = col0."""
        return t[front + self.lay.base:, self.lay.col0:]

    def ptr(self, t, front=0):
        return self.view(t, front).data_ptr()

    def reset(self):
        self.out.copy_(self.out0)
        if hasattr(self, "dqkv"):
            self.dqkv.copy_(self.dqkv0)
            self.part.copy_(self.part0)


# ---- the fp64 statement -------------------------------------------------------------------------------------------------------
def _index(rows, nk, device):
    """Row of (sample, position) clamped into the sample, and which positions are live.  nk: key counts (default: the lengths)."""
    lens = torch.tensor(nk if nk is not None else rows.lens, device=device)
    starts = torch.tensor(rows.starts, device=device)
    pos = torch.arange(max(nk) if nk is not None else rows.L, device=device)
    valid = pos[None, :] < lens[:, None]
    idx = starts[:, None] + torch.minimum(pos[None, :], lens[:, None] - 1)
    return idx, valid


def _gather(view, idx, valid, heads, col):
    """[rows, ...] -> fp64 [B, H, L, 64]; only live rows and the heads' own columns are touched (the rest may be NaN)."""
    B, L = idx.shape
    x = view[idx.reshape(-1), col:col + heads * HD].double().view(B, L, heads, HD).permute(0, 2, 1, 3)
    return torch.where(valid[:, None, :, None], x, torch.zeros((), dtype=torch.float64, device=x.device))


def _scatter(x, idx, valid, live):
    """fp64 [B, H, L, 64] -> [live, H*64] rows."""
    B, H, L, _ = x.shape
    out = torch.zeros(live, H * HD, dtype=torch.float64, device=x.device)
    out[idx[valid]] = x.permute(0, 2, 1, 3).reshape(B, L, H * HD)[valid]
    return out


def operands(qkv, dout, heads, causal, rows, q=None, nkeys=None, row0=0):
    """The operand values of one call as fp64 [B, H, L, 64] tensors.  qkv / dout / q: the block views (Buffers.view); q: the
    compact query rows of a single-query form, whose sample b sees nkeys[b] keys (all of them: no mask)."""
    dev, W = qkv.device, heads * HD
    kidx, kvalid = _index(rows, nkeys, dev)
    p = SimpleNamespace(heads=heads, causal=causal, rows=rows, single=q is not None, kidx=kidx, kvalid=kvalid)
    p.K = _gather(qkv, kidx + row0, kvalid, heads, W)
    p.V = _gather(qkv, kidx + row0, kvalid, heads, 2 * W)
    if q is not None:
        p.Q = q[:rows.n, :W].double().view(rows.n, 1, heads, HD).permute(0, 2, 1, 3)
        p.qvalid = torch.ones(rows.n, 1, dtype=torch.bool, device=dev)
        p.mask = kvalid[:, None, None, :]
        p.dO = None
        return p
    p.Q = _gather(qkv, kidx, kvalid, heads, 0)
    p.qvalid = kvalid
    p.dO = _gather(dout, kidx, kvalid, heads, 0) if dout is not None else None
    L = kidx.shape[1]
    pos = torch.arange(L, device=dev)
    p.mask = kvalid[:, None, None, :] & ((pos[None, :] <= pos[:, None]) if causal else torch.ones(L, L, dtype=torch.bool, device=dev))
    return p


def _softmax(S, mask, qvalid):
    S = S.masked_fill(~mask, -math.inf)
    mx = S.amax(-1, keepdim=True)
    E = torch.exp(S - mx)
    P = E / E.sum(-1, keepdim=True)
    return S, mx, P * qvalid[:, None, :, None]


def _rows_of(p, r, names):
    for n in names:
        x = getattr(r, n)
        setattr(r, n + "_rows", x.permute(0, 2, 1, 3).reshape(p.rows.n, -1) if p.single else _scatter(x, p.kidx, p.kvalid, p.rows.live))


def _colsum(p, r):
    """Per-sample token sums of the dqkv rows, [n, 3*H*64]."""
    f = lambda x: x.sum(2).reshape(p.rows.n, -1)
    return torch.cat([f(r.dQ), f(r.dK), f(r.dV)], 1)


def reference(qkv, dout, heads, causal, rows, q=None, nkeys=None, row0=0, edit=None):
    """What the entry points leave behind, in fp64.  Returns O (and, with dout, dQ, dK, dV, colsum) as [B, H, L, 64] tensors and
    as *_rows [live, heads*64] (single-query forms: [n, heads*64]), the intermediates S, mx, P, dP, delta, dS, and .p, the
    operands.  expected() places the rows into a whole buffer with the `stored` mask.  edit(p): changes the operands or the
    mask first (the CPU test's seeded defects)."""
    p = operands(qkv, dout, heads, causal, rows, q, nkeys, row0)
    if edit is not None:
        edit(p)
    r = SimpleNamespace(p=p)
    r.S, r.mx, r.P = _softmax(p.Q @ p.K.transpose(-1, -2), p.mask, p.qvalid)
    r.O = r.P @ p.V
    names = ["O"]
    if p.dO is not None:
        r.dV = r.P.transpose(-1, -2) @ p.dO
        r.dP = p.dO @ p.V.transpose(-1, -2)
        r.delta = (r.P * r.dP).sum(-1, keepdim=True)
        r.dS = r.P * (r.dP - r.delta)
        r.dQ = r.dS @ p.K
        r.dK = r.dS.transpose(-1, -2) @ p.Q
        r.colsum = _colsum(p, r)
        names += ["dQ", "dK", "dV"]
    _rows_of(p, r, names)
    return r


def bound(r):
    """Per-element error bounds of O, dQ, dK, dV (same shapes as reference()'s *_rows), from the kernels' rounding points.

    First order, u = 2^-9 per bf16 rounding:
      O[q,c]   u (|O| + 2 sum_k P |V|): the forward rounds the exponentials to bf16 for the P V MFMA (u sum P |V|), divides
               by their fp32 sum taken BEFORE that rounding (no first-order term), and stores bf16 (u |O|); the second
               sum P |V| is the issue's allowance for the normalisation not cancelling the operand's rounding.
      dV[k,c]  u (|dV| + sum_q P |dO|): bf16 P as the MFMA operand, bf16 store.
      dQ[q,c]  u (|dQ| + sum_k |dS| |K|), dK[k,c] u (|dK| + sum_q |dS| |Q|): bf16 dS as the operand, bf16 store.
    Second order (the floor: elements such as row 0 of a causal sample have P = 1, dS = 0 and a first-order bound of 0), every
    term propagated through the same sums:
      scores   |dS_| <= E_DOT * max_k sum_c |Q||K|: a 64-term fp32 dot product of exact products.  The worst case is 64
               roundings; sqrt(64) = 8 is taken, because at 64 the term would be first-order in the sharp regimes and an
               MFMA's internal sum is wider than fp32.  It enters P twice (the score and the row maximum).
      exp      relative E_EXP (1 + |s - max|) for __expf, and 2^-22 (|s| + |max|) for the workgroup kernel's
               exp2(fma(s, log2e, -max log2e)), whose argument is rounded at the magnitude of s and max, not of s - max.
      P        rel = the two above; the normaliser carries their P-weighted mean and an N_ACC sum: EP = P (rel + mean + N_ACC).
      dP       E_DOT sum_c |dO||V|;  delta: sum_k (EP |dP| + P EdP) + N_ACC sum_k P |dP|.
      dS       = P (dP - delta) formed in fp32: EP |dP - delta| + P (EdP + Edelta) + 2 EPS32 P (|dP| + |delta|).
      outputs  EP / EdS through the output's own sum, plus N_ACC times that sum of magnitudes (accumulation over <= 288 terms).
      range    fp32 and bf16 share one exponent range; an exponential, a bf16 MFMA operand, a dS or an output below 2^-126 is
               denormal and is flushed to zero or keeps fewer bits (the hardware's choice, the emulation's too): EP, EdS and
               every output bound carry the absolute TINY = 2^-125 (one flush of the fp32 value, one of its bf16 rounding).
               Only the sharp and wide regimes under the causal mask have such elements (a last key only its own query sees)."""
    p, P = r.p, r.P
    aV, aK, aQ = p.V.abs(), p.K.abs(), p.Q.abs()
    live = p.mask & p.qvalid[:, None, :, None]
    zero = torch.zeros((), dtype=torch.float64, device=P.device)
    a = torch.where(live, aQ @ aK.transpose(-1, -2), zero).amax(-1, keepdim=True)
    rel = torch.where(live, E_EXP * (1 + (r.S - r.mx).abs()) + 2.0 ** -22 * (r.S.abs() + r.mx.abs()), zero) + 2 * E_DOT * a
    EP = P * (rel + (P * rel).sum(-1, keepdim=True) + N_ACC) + TINY * live
    PV = P @ aV
    b = SimpleNamespace(p=p)
    b.O = U * (r.O.abs() + 2 * PV) + EP @ aV + N_ACC * PV + TINY
    names = ["O"]
    if p.dO is not None:
        adO, PT = p.dO.abs(), P.transpose(-1, -2)
        PdO = PT @ adO
        b.dV = U * (r.dV.abs() + PdO) + EP.transpose(-1, -2) @ adO + N_ACC * PdO + TINY
        EdP = E_DOT * (adO @ aV.transpose(-1, -2))
        Edelta = (EP * r.dP.abs() + P * EdP).sum(-1, keepdim=True) + N_ACC * (P * r.dP.abs()).sum(-1, keepdim=True)
        EdS = EP * (r.dP - r.delta).abs() + P * (EdP + Edelta) + 2 * EPS32 * P * (r.dP.abs() + r.delta.abs()) + TINY * live
        adS = r.dS.abs()
        SK, SQ = adS @ aK, adS.transpose(-1, -2) @ aQ
        b.dQ = U * (r.dQ.abs() + SK) + EdS @ aK + N_ACC * SK + TINY
        b.dK = U * (r.dK.abs() + SQ) + EdS.transpose(-1, -2) @ aQ + N_ACC * SQ + TINY
        names += ["dQ", "dK", "dV"]
    _rows_of(p, b, names)
    return b


def colsum_bound(dqkv_rows, rows):
    """colsum_part keeps the suite's statement: |part - sum of the STORED rows| <= 2^-8 sum |rows| + 1e-6.  dqkv_rows: the stored
    bf16 rows [live, 3*H*64] -> (expected [n, 3*H*64], bound)."""
    x = dqkv_rows.double()
    seg = [x[s:s + n] for s, n in zip(rows.starts, rows.lens)]
    return torch.stack([s.sum(0) for s in seg]), torch.stack([2.0 ** -8 * s.abs().sum(0) + 1e-6 for s in seg])


def bf16_round(x):
    return x.float().to(BF).double()


def emulate(r, delta_from_o=False, norm_k_shift=0.0):
    """The kernels' rounding points applied to the fp64 statement r = reference(...): the exponentials rounded to bf16 as the
    P V operand and divided by their fp32 sum, bf16 O; bf16 P = fp32 P rounded as dV's operand, fp32 delta from the fp32 P and
    dP, dS formed in fp32 and rounded to bf16 as dQ's and dK's operand, bf16 stores.  Returns O (dQ, dK, dV) like reference().
    The keyword arguments restate one thing wrong each (tests/test_attention_forms_cpu.py)."""
    p = r.p
    f32 = lambda x: x.float().double()
    V = p.V
    S = r.S
    E = f32(torch.exp(S - r.mx)) * p.qvalid[:, None, :, None]
    if norm_k_shift:                                       # the normaliser taken from the scores of k - shift: the offset leaks into P
        S0 = (p.Q @ (p.K - norm_k_shift * p.kvalid[:, None, :, None]).transpose(-1, -2)).masked_fill(~p.mask, -math.inf)
        mx0 = S0.amax(-1, keepdim=True)
        E = f32(torch.exp(S - mx0)) * p.qvalid[:, None, :, None]
        ssum = f32(torch.exp(S0 - mx0)).float().sum(-1, keepdim=True).double()
    else:
        ssum = E.float().sum(-1, keepdim=True).double()
    ssum = torch.where(p.qvalid[:, None, :, None], ssum, torch.ones_like(ssum))       # (padded query rows of a packed sample: E = 0)
    e = SimpleNamespace(p=p)
    e.O = bf16_round((bf16_round(E) @ V) / ssum)
    names = ["O"]
    if p.dO is not None:
        P32 = f32(E / ssum)
        dP = f32(p.dO @ V.transpose(-1, -2))
        if delta_from_o:                                   # the defect csrc/attention_bwd.hip describes: delta from the stored bf16 O
            delta = f32((p.dO * e.O).float().sum(-1, keepdim=True).double())
        else:
            delta = (P32 * dP).float().sum(-1, keepdim=True).double()
        dS = bf16_round(f32(P32 * f32(dP - delta)))
        e.dV = bf16_round(bf16_round(P32).transpose(-1, -2) @ p.dO)
        e.dQ = bf16_round(dS @ p.K)
        e.dK = bf16_round(dS.transpose(-1, -2) @ p.Q)
        names += ["dQ", "dK", "dV"]
    _rows_of(p, e, names)
    return e


# ---- whole buffers ------------------------------------------------------------------------------------------------------------
def expected(prev, layout, values, bnd, nrows_zero=0, front=0):
    """Place the stored rows into a whole buffer: (expected fp64, bound fp64, stored bool), all of prev's shape.  values / bnd:
    [rows, width] starting at the block's first row; nrows_zero rows behind them are stored as exact zeros (the pad rows)."""
    exp, b = prev.double().clone(), torch.zeros(prev.shape, dtype=torch.float64, device=prev.device)
    stored = torch.zeros(prev.shape, dtype=torch.bool, device=prev.device)
    r0, c0, (n, w) = front + layout.base, layout.col0, values.shape
    exp[r0:r0 + n, c0:c0 + w], b[r0:r0 + n, c0:c0 + w] = values, bnd
    exp[r0 + n:r0 + n + nrows_zero, c0:c0 + w] = 0
    stored[r0:r0 + n + nrows_zero, c0:c0 + w] = True
    return exp, b, stored


def worst(got, exp, bnd, stored, prev, parts=None):
    """The worst |got - exp| / bnd over the stored elements of each part (column ranges of the buffer; default: one part, every
    column), as a tensor of len(parts).  A zero bound admits only the exact value.  inf in every part when an element outside
    `stored` changed a bit, nan in a part when one of its stored elements is NaN."""
    bits = lambda t: t.view(torch.int16) if t.dtype == BF else t.view(torch.int32)
    moved = ((bits(got) != bits(prev)) & ~stored).any()
    g = got.double()
    err = (g - exp).abs()
    ratio = torch.where(bnd > 0, err / bnd, torch.where(err == 0, torch.zeros_like(err), torch.full_like(err, math.inf)))
    ratio = torch.where(stored, ratio, torch.zeros_like(ratio))
    isnan = stored & g.isnan()
    ratio = torch.where(isnan, torch.zeros_like(ratio), ratio)
    out = []
    for c0, c1 in parts or [(0, got.shape[1])]:
        w = ratio[:, c0:c1].amax() if c1 > c0 else ratio.new_zeros(())
        w = torch.where(isnan[:, c0:c1].any(), torch.full_like(w, math.nan), w)
        out.append(torch.where(moved & ~w.isnan(), torch.full_like(w, math.inf), w))
    return torch.stack(out)


def thirds(layout, heads):
    W = heads * HD
    return [(layout.col0 + i * W, layout.col0 + (i + 1) * W) for i in range(3)]


def passes(w, kind):
    """w: worst()'s tensor (or a float).  nan and inf fail."""
    return bool((torch.as_tensor(w) <= MARGIN[kind]).all())


def measure_emulation(heads=5):
    """The largest worst-ratio of emulate() over the cases of the GPU sweep (every L and length list, both masks, the four
    regimes): what EMULATION_MAX records.  {"fwd", "lastq", "bwd"}; a few seconds on the CPU."""
    top = {"fwd": 0.0, "lastq": 0.0, "bwd": 0.0}
    ratio = lambda e, r, b, n: float(((getattr(e, n + "_rows") - getattr(r, n + "_rows")).abs() / getattr(b, n + "_rows")).max())
    cases = [Rows.fixed(L, 3) for L in sorted(set(FWD_L + BWD_L))] + [Rows(lens, True, 9) for lens in PACKED]
    for rows in cases:
        for causal in (False, True):
            for regime in REGIMES:
                d = make_data(rows, heads, regime, 7 * rows.L + causal)
                r = reference(d.qkv, d.dout, heads, causal, rows)
                b, e = bound(r), emulate(r)
                top["fwd"] = max(top["fwd"], ratio(e, r, b, "O"))
                if rows.L <= max(BWD_L):
                    top["bwd"] = max(top["bwd"], *(ratio(e, r, b, n) for n in ("dQ", "dK", "dV")))
    single = [(Rows.fixed(L, 3), nk) for L in LASTQ_L for nk in ([L] * 3, [max(L - 3, 1), 1, L])]
    for rows, nkeys in single + [(Rows(lens, True), list(lens)) for lens in LASTQ_PACKED]:
        for regime in REGIMES:
            d = make_data(rows, heads, regime, rows.L, nq=rows.n)
            r = reference(d.qkv, None, heads, False, rows, q=d.qc, nkeys=nkeys)
            top["lastq"] = max(top["lastq"], ratio(emulate(r), r, bound(r), "O"))
    return top


if __name__ == "__main__":
    print(measure_emulation())
