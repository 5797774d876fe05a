"""Exact operands, float64 reference and case table of the convolution family (tests/test_conv_exact_cases.py checks this module
without a GPU, tests/test_gpu_conv_exact.py runs the table on the device).  No GPU is needed to import or use it.

EXACT OPERANDS.  Every operand is a seeded integer draw times a power of two:

    x = a 2^-2, |a| <= 7 (a quarter of the draws forced to 0)        w = b 2^-1, |b| <= 3
    bias = c 2^-1, |c| <= 8                                            residual = r 2^-2, |r| <= 31

so every product x w is an integer multiple of the QUANTUM 2^-3, and so are bias and residual.  A sum of such terms whose
magnitudes add up to less than 2^24 quanta is an integer below 2^24 times 2^-3: an fp32 number.  The BUDGET of a case,

    budget = max over outputs of ( sum |x| |w| + |bias| + |residual| ) / 2^-3          (`budget(case)`)

bounds EVERY partial sum a kernel can form from the terms of one output, in any order and any grouping (k-tiles, split-K
slices, MFMA trees, bf16 pieces - a piece of an operand is no larger than the operand and a multiple of its quantum), so below
2^24 all of them are exact, no rounding ever happens, and the fp32 result IS the real number: `conv_ref(case).astype(float32)` is
lossless and a kernel must return it bit for bit.  These operands have at most 5 significant bits and are fp16 numbers too, so
the fp16 routes multiply the same values, accumulate them exactly in fp32, and an fp16 output is ONE round-to-nearest-even of
the exact value: `conv_ref(case).astype(float16)`.

WIDE rows, on the routes that split or round their operands, draw x = a 2^-6 with |a| <= 511 and w = b 2^-(k-1) with
|b| < 2^k instead: k = 9 on the 1x1 kernels, so that x and w are each MORE than one bf16 piece and the middle pieces and their
cross products carry real bits; k = 5 on the fp16 entries' 3x3 layers, whose longer K leaves less room.  Nine significant bits
are still an fp16 number.  Their quantum is 2^-(k+5) (`case.quantum`; bias and residual are multiples of it), and the same
argument holds with it: budget below 2^24 quanta, every partial sum exact.

F(2x2,3x3) WINOGRAD sums other terms, so it gets its own budget (`budget_f22(case)`), derived from the matrices csrc/winograd.hip
uses - Y = At [ sum_c (G g Gt) . (Bt d B) ] A with

    Bt = [1 0 -1 0; 0 1 1 0; 0 -1 1 0; 0 1 0 -1]    (row_piece / col_piece: integer, applied in the kernel to the raw 4x4 patch)
    G  = [1 0 0; 1/2 1/2 1/2; 1/2 -1/2 1/2; 0 0 1]  (both factors of 1/2 sit in the WEIGHT transform, *_pack_weights_kernel,
                                                      computed in double and stored as fp32; none in Bt or At)
    At = [1 1 1 0; 0 1 -1 -1]                       (epilogue: m0 + m1 + m2, m1 - m2 - m3, integer)

V = Bt d B is a signed sum of 4 inputs: an integer number of x quanta (2^-2), |V| <= 28 quanta - exact.  U = G g Gt has
quantum 2^-1 / 4 = 2^-3 and |U| <= (3/2)^2 max|w| = 27 quanta - exact in double and in fp32.  The 16 products per input
channel have quantum 2^-5; an output is a signed sum of 9 of the 16 M_xi = sum_c V_xi U_xi, and every intermediate the kernel
forms (the k-loop of one xi, its row fold, the column fold, + bias, + residual) is a partial sum of those terms, so

    budget_f22 = max over tiles and output channels of ( sum_xi sum_c |V_xi| |U_xi| + |bias| + |residual| ) / 2^-5

below 2^24 makes the F(2x2) kernels exact as well, and they are held to bit equality.

F(4x4,3x3) CANNOT be exact on dyadic data: csrc/winograd43.hip interpolates at (0, 3/4, -3/4, 3/2, -3/2, inf), and the rows of
its G are (1, p, p^2) / prod_{q != p} (p - q); for p = 3/4 the denominator is (3/4)(3/2)(-3/4)(9/4) = -243/128, so U carries
factors of 1/3 that no power-of-two scaling of the weights removes, and U is rounded to fp32 when it is packed.  Those rows are
held to the bounds the project states for the kernel (2e-5 of the output range for the single-launch forms, 1e-5 for split-K,
tests/test_gpu_f_ops.py) - here against a reference that is itself exact - and to run-to-run bit identity.

CASE TABLE.  One row per (route, option set), written from the descriptor contract in include/glass_hip.h and the
*_supported() predicates; `ROUTE_ROWS` repeats the number of rows per route as literals so that a route cannot lose rows
silently.  A row names how the route is forced (conv2d_nhwc's `winograd` / `f43k`, Routing fields, the `_splitk_slices`
substitution), the last_conv_path() and library entry the launch must take, and whether the route ACCEPTS the option set; a
refused row names the path that takes the layer instead, and that launch is held to the same standard."""
import dataclasses
import functools
import zlib
from typing import Optional

import numpy as np

X_Q, W_Q, B_Q, R_Q = 2.0 ** -2, 2.0 ** -1, 2.0 ** -1, 2.0 ** -2
X_MAX, W_MAX, B_MAX, R_MAX = 7, 3, 8, 31
QUANTUM = X_Q * W_Q                 # 2^-3: products, bias and residual are integer multiples of it
QUANTUM_F22 = X_Q * W_Q / 4.0       # 2^-5: products in the F(2x2) transform domain
WIDE_X_MAX, WIDE_X_Q = 511, 2.0 ** -6       # wide rows: 9-bit x (two bf16 pieces, exact in fp16) and `wide`-bit w = b 2^-(wide-1)
BUDGET_LIMIT = float(1 << 24)
PAD = 8                             # extra channels of a wider x / residual / output pixel: keeps every stride a multiple of 16 bytes
F43_BOUND, F43K_BOUND = 2e-5, 1e-5  # of the output range: the project's bounds for the F(4x4) single-launch / split-K forms

D, DK = "glass_conv2d_nhwc", "glass_conv2d_nhwc_splitk"
W22, W22B = "glass_conv3x3_winograd_nhwc", "glass_conv3x3_winograd_body_nhwc"
W43, W43B, W43R, W43K = ("glass_conv3x3_winograd43_nhwc", "glass_conv3x3_winograd43_body_nhwc",
                         "glass_conv3x3_winograd43_ragged_nhwc", "glass_conv3x3_winograd43_splitk_nhwc")
PW, PWS, DUAL = "glass_conv1x1_pointwise_nhwc", "glass_conv1x1_pointwise_split_nhwc", "glass_conv1x1_pointwise_split_dual_nhwc"
F16, H16, H16P = "glass_conv2d_nhwc_f16", "glass_conv2d_nhwc_h16", "glass_conv2d_nhwc_h16_packed"
BSTEM, LSTEM = "glass_backbone_stem_fused", "glass_local_stem_fused"

# the routing every row starts from (explicit, so that no GLASS_* environment variable changes what a row forces)
BASE_ROUTING = dict(precision="fp32", winograd=True, f43=True, pw=True, h16=True, local_stem=True, stem=True, ragged="tiles",
                    pooled_fusion=True, rnn="1x1", splitk=True, small_grid=True, split=9)


@dataclasses.dataclass(frozen=True)
class Case:
    id: str
    route: str
    fn: str                       # "conv" | "linear" | "dual" | "backbone_stem" | "local_stem"
    N: int
    H: int
    W: int
    Cin: int
    Cout: int
    KH: int = 1
    KW: int = 1
    stride: tuple = (1, 1)
    pad: tuple = (0, 0)
    ldx_pad: int = 0              # x is the first Cin of Cin + ldx_pad channels
    ldr_pad: int = 0              # the residual is the first Cout of Cout + ldr_pad channels
    y_coff: int = 0
    y_cstride: int = 1
    ldy_tail: int = 0             # channels of an output pixel behind the window
    relu: int = 0
    res_mode: int = 0
    bias: bool = True
    Cin2: int = 0                 # dual-source kernel: channels of the second source
    wide: int = 0                 # wide rows: significant bits of w (x has 9; module docstring)
    # ---- how the route is forced
    forced: object = None         # conv2d_nhwc(winograd=...)
    f43k: object = None           # conv2d_nhwc(f43k=...)
    routing: tuple = ()           # (field, value) pairs replacing BASE_ROUTING fields
    slices: Optional[int] = None  # substituted for ops.native._splitk_slices (None: the rule itself)
    half: int = 0                 # fp16 storage: bit 0 x, bit 1 y, bit 2 residual (the flags of glass_conv2d_nhwc_h16)
    # ---- what must happen
    path: str = "direct"          # last_conv_path()
    entry: str = D                # the library entry of the launch
    strip: bool = False           # ... followed by the last-column strip convolution
    accepts: bool = True          # the route's predicate takes this option set (False: `path` / `entry` name the fallback)
    predicate: Optional[str] = None   # the route's *_supported() (None: the implicit-GEMM entries take every valid descriptor)
    refused_forced: object = None     # refused rows of a route forced through `winograd=`: the value that must raise
    exact: bool = True            # False: an F(4x4) launch, held to `bound` of the output range
    bound: float = 0.0

    @property
    def quantum(self):
        return WIDE_X_Q * 2.0 ** -(self.wide - 1) if self.wide else QUANTUM

    @property
    def ldx(self):
        return self.Cin + self.ldx_pad

    @property
    def ldr(self):
        return self.Cout + self.ldr_pad if self.res_mode else 0

    @property
    def ldy(self):
        return self.y_coff + (self.Cout - 1) * self.y_cstride + 1 + self.ldy_tail

    @property
    def out_hw(self):
        return ((self.H + 2 * self.pad[0] - self.KH) // self.stride[0] + 1, (self.W + 2 * self.pad[1] - self.KW) // self.stride[1] + 1)

    @property
    def res_hw(self):
        Ho, Wo = self.out_hw
        return (Ho // 2, Wo // 2) if self.res_mode == 2 else (Ho, Wo)

    def desc_ints(self):
        """the 20 ints of glass_conv_desc / ops.native.ConvDesc, as conv2d_nhwc fills them"""
        Ho, Wo = self.out_hw
        return (self.N, self.H, self.W, self.Cin, self.Cout, self.KH, self.KW, *self.stride, *self.pad, Ho, Wo, self.ldx, self.ldy,
                self.y_coff, self.y_cstride, self.relu, self.res_mode, self.ldr)


# ================================================================================================ operands and reference
def _rng(case, salt):
    return np.random.default_rng(zlib.crc32(f"{case.id}/{salt}".encode()))


@functools.lru_cache(maxsize=None)
def operands(case):
    """-> dict of float64 arrays, the PADDED buffers the descriptor describes: x [N,H,W,ldx], w [Cout,KH,KW,Cin], bias [Cout] or
    None, res [N,Hr,Wr,ldr] or None (x2 [N,Ho,Wo,Cin2] for the dual kernel).  Channels of x at and beyond Cin and of the residual
    at and beyond Cout are NaN: the contract says they are not read.  (fused stems: the arrays of `stem_operands`.)"""
    def draw(salt, shape, amax, q, zeros=0.0):
        g = _rng(case, salt)
        v = g.integers(-amax, amax + 1, size=shape).astype(np.float64)
        if zeros:
            v[g.random(size=shape) < zeros] = 0.0
        return v * q
    Ho, Wo = case.out_hw
    x = np.full((case.N, case.H, case.W, case.ldx), np.nan)
    (xm, xq), (wm, wq) = ((WIDE_X_MAX, WIDE_X_Q), ((1 << case.wide) - 1, 2.0 ** -(case.wide - 1))) if case.wide else ((X_MAX, X_Q), (W_MAX, W_Q))
    x[..., :case.Cin] = draw("x", (case.N, case.H, case.W, case.Cin), xm, xq, zeros=0.25)
    ops = {"x": x, "w": draw("w", (case.Cout, case.KH, case.KW, case.Cin + case.Cin2), wm, wq),
           "bias": draw("b", (case.Cout,), B_MAX, B_Q) if case.bias else None, "res": None}
    if case.Cin2:
        ops["x2"] = draw("x2", (case.N, Ho, Wo, case.Cin2), xm, xq, zeros=0.25)
    if case.res_mode:
        r = np.full((case.N, *case.res_hw, case.ldr), np.nan)
        r[..., :case.Cout] = draw("r", (case.N, *case.res_hw, case.Cout), R_MAX, R_Q)
        ops["res"] = r
    for v in ops.values():
        if v is not None:
            v.setflags(write=False)
    return ops


def _taps(case, x, w, absolute=False):
    """sum over taps and channels of x w (or |x| |w|) in float64: x [N,H,W,C] dense, w [Cout,KH,KW,C] -> [N,Ho,Wo,Cout]"""
    if absolute:
        x, w = np.abs(x), np.abs(w)
    (sh, sw), (ph, pw), (Ho, Wo) = case.stride, case.pad, case.out_hw
    xp = np.zeros((case.N, case.H + 2 * ph, case.W + 2 * pw, x.shape[3]))
    xp[:, ph:ph + case.H, pw:pw + case.W] = x
    y = np.zeros((case.N, Ho, Wo, w.shape[0]))
    for kh in range(case.KH):
        for kw in range(case.KW):
            y += xp[:, kh:kh + (Ho - 1) * sh + 1:sh, kw:kw + (Wo - 1) * sw + 1:sw] @ w[:, kh, kw].T
    return y


def _residual(case, ops):
    """the residual as the output sees it: the first Cout of ldr channels, x2 nearest-upsampled for res_mode 2"""
    r = ops["res"][..., :case.Cout]
    return r.repeat(2, axis=1).repeat(2, axis=2) if case.res_mode == 2 else r


def conv_ref(case, ops=None):
    """The descriptor contract restated in float64 from the padded buffers: y = act(conv(x[..., :Cin], w) + bias [+ residual]) as
    [N,Ho,Wo,Cout]; relu 1 = after everything, 2 = before the residual add; res_mode 1 = same-shape residual, 2 = the
    [N,Ho/2,Wo/2,ldr] residual nearest-upsampled x2; the residual's first Cout of ldr channels."""
    if case.fn in ("backbone_stem", "local_stem"):
        return stem_ref(case, ops)
    ops = ops or operands(case)
    x = ops["x"][..., :case.Cin]
    w = ops["w"]
    if case.Cin2:                   # y = act([x1 strided | x2] . [W1 | W2]^T + bias): two 1x1 convolutions into one sum
        c2 = dataclasses.replace(case, H=case.out_hw[0], W=case.out_hw[1], stride=(1, 1))
        y = _taps(case, x, w[..., :case.Cin]) + _taps(c2, ops["x2"], w[..., case.Cin:])
    else:
        y = _taps(case, x, w)
    if ops["bias"] is not None:
        y = y + ops["bias"]
    if case.relu == 2:
        y = np.maximum(y, 0.0)
    if case.res_mode:
        y = y + _residual(case, ops)
    if case.relu == 1:
        y = np.maximum(y, 0.0)
    return y


def budget(case, ops=None):
    """max over outputs of sum |x||w| + |bias| + |residual|, in quanta (2^-3; wide rows: `case.quantum`; module docstring); fused stems:
    `stem_budget`"""
    if case.fn in ("backbone_stem", "local_stem"):
        return stem_budget(case, ops)
    ops = ops or operands(case)
    if case.N == 0:
        return 0.0
    s = _taps(case, ops["x"][..., :case.Cin], ops["w"][..., :case.Cin], absolute=True)
    if case.Cin2:
        c2 = dataclasses.replace(case, H=case.out_hw[0], W=case.out_hw[1], stride=(1, 1))
        s = s + _taps(c2, ops["x2"], ops["w"][..., case.Cin:], absolute=True)
    if ops["bias"] is not None:
        s = s + np.abs(ops["bias"])
    if case.res_mode:
        s = s + np.abs(_residual(case, ops))
    return float(s.max()) / case.quantum


F22_BT = np.array([[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]], dtype=np.float64)
F22_G = np.array([[1, 0, 0], [0.5, 0.5, 0.5], [0.5, -0.5, 0.5], [0, 0, 1]], dtype=np.float64)
F22_AT = np.array([[1, 1, 1, 0], [0, 1, -1, -1]], dtype=np.float64)


def f22_transforms(case, ops=None):
    """-> V [N,TH,TW,4,4,Cin] = Bt d B of every 2x2 output tile's 4x4 patch, U [Cout,4,4,Cin] = G g Gt (float64)"""
    ops = ops or operands(case)
    x = ops["x"][..., :case.Cin]
    TH, TW = (case.H + 1) // 2, (case.W + 1) // 2
    xp = np.zeros((case.N, 2 * TH + 2, 2 * TW + 2, case.Cin))
    xp[:, 1:1 + case.H, 1:1 + case.W] = x
    d = np.stack([np.stack([xp[:, r:r + 2 * TH:2, c:c + 2 * TW:2] for c in range(4)], axis=3) for r in range(4)], axis=3)
    V = np.einsum("ir,nhwrck,jc->nhwijk", F22_BT, d, F22_BT)
    U = np.einsum("ia,oabk,jb->oijk", F22_G, ops["w"], F22_G)
    return V, U


def f22_apply(case, ops=None):
    """the F(2x2,3x3) algorithm itself in float64 (before bias): At [sum_c U . V] A, cropped to [N,H,W,Cout]"""
    V, U = f22_transforms(case, ops)
    M = np.einsum("nhwijk,oijk->nhwijo", V, U)
    Y = np.einsum("ai,nhwijo,bj->nhawbo", F22_AT, M, F22_AT)
    N, TH, _, TW, _, Co = Y.shape
    return Y.reshape(N, 2 * TH, 2 * TW, Co)[:, :case.H, :case.W]


def budget_f22(case, ops=None):
    """the transformed-domain budget of the F(2x2,3x3) kernels in quanta of 2^-5 (module docstring)"""
    ops = ops or operands(case)
    if case.N == 0:
        return 0.0
    V, U = f22_transforms(case, ops)
    s = np.einsum("nhwijk,oijk->nhwo", np.abs(V), np.abs(U))          # [N,TH,TW,Cout]
    extra = np.zeros(())
    if ops["bias"] is not None:
        extra = extra + np.abs(ops["bias"]).max()
    if case.res_mode:
        extra = extra + np.abs(_residual(case, ops)).max()
    return float(s.max() + extra) / QUANTUM_F22


def is_f22(case):
    return case.entry in (W22, W22B)


# ------------------------------------------------------------------------------------------------ fused stems
def _maxpool(y, k, s, p):
    N, H, W, C = y.shape
    Ho, Wo = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    yp = np.full((N, H + 2 * p, W + 2 * p, C), -np.inf)
    yp[:, p:p + H, p:p + W] = y
    out = np.full((N, Ho, Wo, C), -np.inf)
    for a in range(k):
        for b in range(k):
            out = np.maximum(out, yp[:, a:a + (Ho - 1) * s + 1:s, b:b + (Wo - 1) * s + 1:s])
    return out


def _stem_layers(case):
    """the convolutions a fused stem chains, as Cases over dense operands"""
    if case.fn == "backbone_stem":      # 7x7 stride 2 pad 3, 3 -> 64 (+ ReLU), then max-pool 3x3 stride 2 pad 1
        return (dataclasses.replace(case, fn="conv", Cin=3, Cout=64, KH=7, KW=7, stride=(2, 2), pad=(3, 3), relu=1),)
    c1 = dataclasses.replace(case, fn="conv", Cin=4, Cout=16, KH=3, KW=3, pad=(1, 1), relu=1)
    return (c1, dataclasses.replace(c1, Cin=16, Cout=32))          # ... then max-pool 2x2


@functools.lru_cache(maxsize=None)
def stem_operands(case):
    """backbone stem: x [N,H,W,4] whose 4th channel is NaN (the contract: ignored), w [64,7,7,4] (w[..., 3] ignored too), bias;
    local stem: x [R,H,W,4] NHWC4 crops whose 4th channel is 0 (what the preprocessing writes), w1 [16,3,3,4], b1, w2 [32,3,3,16], b2"""
    g = _rng(case, "stem")
    def draw(shape, amax, q):
        return g.integers(-amax, amax + 1, size=shape).astype(np.float64) * q
    x = draw((case.N, case.H, case.W, 4), X_MAX, X_Q)
    x[g.random(size=x.shape) < 0.25] = 0.0
    if case.fn == "backbone_stem":
        x[..., 3] = np.nan if case.accepts else 0.0      # (the refused row runs the separate entries, which read all 4 channels)
        ops = {"x": x, "w": draw((64, 7, 7, 4), W_MAX, W_Q), "bias": draw((64,), B_MAX, B_Q)}
    else:
        x[..., 3] = 0.0
        ops = {"x": x, "w1": draw((16, 3, 3, 4), W_MAX, W_Q), "b1": draw((16,), B_MAX, B_Q),
               "w2": draw((32, 3, 3, 16), W_MAX, W_Q), "b2": draw((32,), B_MAX, B_Q)}
    for v in ops.values():
        v.setflags(write=False)
    return ops


def stem_ref(case, ops=None):
    ops = ops or stem_operands(case)
    if case.fn == "backbone_stem":
        (c,) = _stem_layers(case)
        y = np.maximum(_taps(c, ops["x"][..., :3], ops["w"][..., :3]) + ops["bias"], 0.0)
        return _maxpool(y, 3, 2, 1)
    c1, c2 = _stem_layers(case)
    a1 = np.maximum(_taps(c1, ops["x"], ops["w1"]) + ops["b1"], 0.0)
    a2 = np.maximum(_taps(c2, a1, ops["w2"]) + ops["b2"], 0.0)
    return _maxpool(a2, 2, 2, 0)


def stem_budget(case, ops=None):
    """the larger of the chained convolutions' budgets, each in its own quantum: 2^-3 for a first layer, 2^-4 for conv0_2 (its
    input, the conv0_1 map, has quantum 2^-3; the weights 2^-1); a max-pool returns one of its inputs"""
    ops = ops or stem_operands(case)
    if case.N == 0:
        return 0.0
    if case.fn == "backbone_stem":
        (c,) = _stem_layers(case)
        return float((_taps(c, ops["x"][..., :3], ops["w"][..., :3], absolute=True) + np.abs(ops["bias"])).max()) / QUANTUM
    c1, c2 = _stem_layers(case)
    b1 = float((_taps(c1, ops["x"], ops["w1"], absolute=True) + np.abs(ops["b1"])).max()) / QUANTUM
    a1 = np.maximum(_taps(c1, ops["x"], ops["w1"]) + ops["b1"], 0.0)
    b2 = float((_taps(c2, a1, ops["w2"], absolute=True) + np.abs(ops["b2"])).max()) / (QUANTUM * W_Q)
    return max(b1, b2)


# ================================================================================================ option sets
# (what a row changes in the plain descriptor; RES / RELU2 carry a residual so that the ReLU's position changes the result)
PLAIN = {}
LDX = dict(ldx_pad=PAD)
LDR = dict(res_mode=1, ldr_pad=PAD)
WINDOW = dict(y_coff=PAD, ldy_tail=PAD)
RES1 = dict(res_mode=1)
RES2 = dict(res_mode=2)
RELU1 = dict(relu=1, res_mode=1)
RELU2 = dict(relu=2, res_mode=1)
NOBIAS = dict(bias=False)
CSTRIDE2 = dict(y_cstride=2, y_coff=1, ldy_tail=3)
ALL1 = dict(ldx_pad=PAD, ldr_pad=PAD, y_coff=PAD, ldy_tail=PAD, relu=2, res_mode=1)
ALL2 = dict(ldx_pad=PAD, ldr_pad=PAD, y_coff=PAD, ldy_tail=PAD, relu=1, res_mode=2)
# ... and everything at once on the SCALAR epilogue of the implicit-GEMM entries (a channel step of 2; csrc/conv.hip takes it too
# when Cout % 4 != 0): its own residual addressing, ReLU positions and fp16 conversions
ALL1C = dict(ldx_pad=PAD, ldr_pad=PAD, y_cstride=2, y_coff=1, ldy_tail=3, relu=2, res_mode=1)
ALL2C = dict(ldx_pad=PAD, ldr_pad=PAD, y_cstride=2, y_coff=1, ldy_tail=3, relu=1, res_mode=2)
N0 = dict(N=0)
WIDE = [("wide", dict(wide=9)), ("wide-all1", dict(ALL1, wide=9)), ("wide-all2", dict(ALL2, wide=9))]
WIDE5 = [(n, dict(o, wide=5)) for n, o in WIDE]

CASES = []


def _rows(route, shape, force, expect, rows):
    """rows of one route: (option-set name, option set[, refusal]) - a refusal is the dict of what happens instead
    (accepts=False, the fallback's path / entry / forcing)"""
    for name, opts, *refusal in rows:
        kw = dict(shape)
        kw.update(force)
        kw.update(expect)
        kw.update(opts)
        if refusal:
            kw.update(accepts=False, strip=False, exact=True, bound=0.0)
            kw.update(refusal[0])
        CASES.append(Case(id=f"{route}-{name}", route=route, **kw))


def _to_direct(**kw):
    """refused by a route forced through `winograd=`: that call raises; the direct kernel (winograd=False) takes the layer"""
    return dict(path="direct", entry=D, forced=False, f43k=None, routing=(("splitk", False),), **kw)


# ------------------------------------------------------------------------------------------------ direct implicit GEMM
# glass_conv2d_nhwc takes every valid descriptor (no predicate); tiles BM x BN of conv_dispatch, k-tiles of 32
_DIRECT = dict(fn="conv", forced=False, routing=(("splitk", False),))
_DIRECT_OK = dict(path="direct", entry=D)
_DIRECT_ROWS = [("plain", PLAIN), ("ldx", LDX), ("ldr", LDR), ("window", WINDOW), ("res1", RES1), ("res2", RES2), ("relu1", RELU1),
                ("relu2", RELU2), ("nobias", NOBIAS), ("cstride2", CSTRIDE2), ("all1", ALL1), ("all2", ALL2), ("n0", N0),
                ("all1-cstride2", ALL1C), ("all2-cstride2", ALL2C)]
# Cout <= 32: 128 x 32 tiles; 3x3 16 -> 32 on 2 x 10 x 8 = 160 pixels (2 row blocks, the last ragged), Ktot 144 = 5 k-tiles that
# straddle taps (Cin % 32 != 0: the per-chunk tap decode)
_rows("direct-128x32", dict(N=2, H=10, W=8, Cin=16, Cout=32, KH=3, KW=3, pad=(1, 1)), _DIRECT, _DIRECT_OK, _DIRECT_ROWS)
# Cout <= 64: 128 x 64 tiles; the 7x7 / stride 2 / pad 3 stem layer, Cin 4: 23 x 27 -> 12 x 14 = 168 pixels, Ktot 196 = 7 k-tiles
_rows("direct-stem7x7", dict(N=1, H=23, W=27, Cin=4, Cout=64, KH=7, KW=7, stride=(2, 2), pad=(3, 3)), _DIRECT, _DIRECT_OK, _DIRECT_ROWS)
# ... Cin 36 (not a multiple of 32) and Cout 40 (a ragged channel block): 3x3 on 8 x 18 = 144 pixels, Ktot 324 = 11 k-tiles.
# Cout 40 is a multiple of 4 and still takes the vector epilogue; Cout 42 does not: every option set on the scalar epilogue
_rows("direct-cin36-cout40", dict(N=1, H=8, W=18, Cin=36, Cout=40, KH=3, KW=3, pad=(1, 1)), _DIRECT, _DIRECT_OK, _DIRECT_ROWS)
_rows("direct-cin36-cout42", dict(N=1, H=8, W=18, Cin=36, Cout=42, KH=3, KW=3, pad=(1, 1)), _DIRECT, _DIRECT_OK, _DIRECT_ROWS)
# ... the 2x2 stride-(2,1) and 2x1 stride-(2,1) layers of the local extractor: 32 -> 64, 3 x 16 x 9 -> 8 x 8 (192 pixels) and
# 4 x 8 x 10 -> 4 x 10 (160 pixels); 4 and 2 k-tiles, one tap each (Cin % 32 == 0: the uniform-tap loads)
_rows("direct-2x2s21", dict(N=3, H=16, W=9, Cin=32, Cout=64, KH=2, KW=2, stride=(2, 1)), _DIRECT, _DIRECT_OK, _DIRECT_ROWS)
_rows("direct-2x1s21", dict(N=4, H=8, W=10, Cin=32, Cout=64, KH=2, KW=1, stride=(2, 1)), _DIRECT, _DIRECT_OK, _DIRECT_ROWS)
# Cout <= 96: 128 x 96 tiles; 1x1 64 -> 72 on 3 x 8 x 6 = 144 pixels, 2 k-tiles
_rows("direct-128x96", dict(N=3, H=8, W=6, Cin=64, Cout=72), _DIRECT, _DIRECT_OK, _DIRECT_ROWS)
# Ktot <= 256: 64 x 64 tiles; 1x1 64 -> 136 (3 channel blocks, the last ragged) on 6 x 14 = 84 pixels (2 row blocks)
_rows("direct-k256-64x64", dict(N=1, H=6, W=14, Cin=64, Cout=136), _DIRECT, _DIRECT_OK, _DIRECT_ROWS)
# few rows, Cout >= 256, Ktot > 256: 64 x 64 tiles again; 3x3 32 -> 256, Ktot 288 = 9 k-tiles
_rows("direct-fewtile-64x64", dict(N=1, H=6, W=14, Cin=32, Cout=256, KH=3, KW=3, pad=(1, 1)), _DIRECT, _DIRECT_OK, _DIRECT_ROWS)
# 96 < Cout < 256, Ktot > 256, few tiles: 64 x 128 tiles; 3x3 32 -> 160 (2 channel blocks, the last ragged)
_rows("direct-64x128", dict(N=1, H=6, W=14, Cin=32, Cout=160, KH=3, KW=3, pad=(1, 1)), _DIRECT, _DIRECT_OK, _DIRECT_ROWS)
# >= 640 tiles of 128 x 128: 3x3 32 -> 128 on 286 x 288 = 82368 pixels (644 row blocks, the last ragged) - the one big case
_rows("direct-128x128", dict(N=1, H=286, W=288, Cin=32, Cout=128, KH=3, KW=3, pad=(1, 1)), _DIRECT, _DIRECT_OK,
      [("plain", PLAIN), ("all1", ALL1), ("all2", ALL2), ("all1-cstride2", ALL1C)])

# ------------------------------------------------------------------------------------------------ direct split-K
# glass_conv2d_nhwc_splitk, 3 slices substituted for the cost model: 3x3 32 -> 64 (64 x 64 tiles) and 32 -> 24 (128 x 32 tiles) on
# 3 x 6 x 10 = 180 pixels, 9 k-tiles = 3 per slice; window, residual, ReLU and the channel step go through the reducer
_SPLITK = dict(fn="conv", forced=False, slices=3, predicate="glass_conv2d_splitk_supported")
_SPLITK_OK = dict(path="direct", entry=DK)
_SPLITK_ROWS = [("plain", PLAIN), ("ldx", LDX), ("ldr", LDR), ("window", WINDOW), ("res1", RES1),
                ("res2", RES2, dict(path="direct", entry=D)),          # res_mode 0/1 only: the single-slice kernel
                ("relu1", RELU1), ("relu2", RELU2), ("nobias", NOBIAS), ("cstride2", CSTRIDE2), ("all1", ALL1),
                ("all1-cstride2", ALL1C),
                ("n0", N0, dict(path="direct", entry=D))]              # no output pixels: nothing to split
_rows("splitk-64x64", dict(N=3, H=6, W=10, Cin=32, Cout=64, KH=3, KW=3, pad=(1, 1)), _SPLITK, _SPLITK_OK, _SPLITK_ROWS)
_rows("splitk-128x32", dict(N=3, H=6, W=10, Cin=32, Cout=24, KH=3, KW=3, pad=(1, 1)), _SPLITK, _SPLITK_OK, _SPLITK_ROWS)

# ------------------------------------------------------------------------------------------------ F(2x2,3x3) Winograd
# glass_winograd_supported: 3x3 s1 p1, Cin % 16, Cout % 64, unit channel step, ldx / ldy / y_coff / ldr % 4, res_mode 0/1
_F22 = dict(fn="conv", KH=3, KW=3, pad=(1, 1), forced=True, predicate="glass_winograd_supported")
_F22_ROWS = [("plain", PLAIN), ("ldx", LDX), ("ldr", LDR), ("window", WINDOW), ("res1", RES1),
             ("res2", RES2, _to_direct(refused_forced=True)), ("relu1", RELU1), ("relu2", RELU2), ("nobias", NOBIAS),
             ("cstride2", CSTRIDE2, _to_direct(refused_forced=True)), ("all1", ALL1), ("n0", N0)]
# 64-tile x 64-channel blocks, k-tiles of 16: 32 -> 64 on 3 x 10 x 12 (90 tiles: 2 blocks, the last ragged), 2 k-tiles;
# 32-tile x 128-channel blocks, k-tiles of 32: 64 -> 128 on 2 x 10 x 12 (60 tiles: 2 blocks), 2 k-tiles
_rows("f22-64", dict(N=3, H=10, W=12, Cin=32, Cout=64), _F22, dict(path="winograd", entry=W22), _F22_ROWS)
_rows("f22-128", dict(N=2, H=10, W=12, Cin=64, Cout=128), _F22, dict(path="winograd128", entry=W22), _F22_ROWS)
# the 1 x 3 x 5 map (odd height and width, one ragged block, a single k-tile)
_rows("f22-1x3x5", dict(N=1, H=3, W=5), _F22, {},
      [("64", dict(Cin=16, Cout=64, path="winograd", entry=W22)), ("128", dict(Cin=32, Cout=128, path="winograd128", entry=W22)),
       ("64-all1", dict(Cin=16, Cout=64, path="winograd", entry=W22, **ALL1)),
       ("128-all1", dict(Cin=32, Cout=128, path="winograd128", entry=W22, **ALL1))])
# forced "f22r": the full tile columns + the last column as a strip convolution (KH 3, KW 1 over the last two columns seen as 2 Cin
# channels - needs dense rows, ldx == Cin, which plan_conv checks itself: no library predicate refuses a wider pixel here)
_F22R = dict(fn="conv", KH=3, KW=3, pad=(1, 1), forced="f22r", predicate="glass_winograd_supported", strip=True)
# (res_mode 2 cannot be asked of the odd-width forms at all - here, the ragged and body forms and the split-K body form: an
#  upsampled residual needs an even Wo, so no entry takes such a descriptor and there is no fallback to name)
_F22R_ROWS = [("plain", PLAIN), ("ldx", LDX, _to_direct(refused_forced="f22r", predicate=None)), ("ldr", LDR), ("window", WINDOW),
              ("res1", RES1), ("relu1", RELU1), ("relu2", RELU2), ("nobias", NOBIAS), ("all1", dict(ALL1, ldx_pad=0)),
              ("cstride2", CSTRIDE2, _to_direct(refused_forced="f22r")),
              ("n0", N0, _to_direct(refused_forced="f22r", predicate=None))]       # plan_conv: no strip without pixels
_rows("f22r-64", dict(N=2, H=3, W=5, Cin=16, Cout=64), _F22R, dict(path="winogradr", entry=W22B), _F22R_ROWS)
_rows("f22r-128", dict(N=3, H=6, W=5, Cin=32, Cout=128), _F22R, dict(path="winograd128r", entry=W22B), _F22R_ROWS)

# ------------------------------------------------------------------------------------------------ F(4x4,3x3) Winograd
# glass_winograd43_supported: as the F(2x2) predicate (ldx % 2).  Not exact (module docstring): `bound` of the output range.
_F43 = dict(fn="conv", KH=3, KW=3, pad=(1, 1), forced="f43", predicate="glass_winograd43_supported", exact=False, bound=F43_BOUND)
_F43_ROWS = [("plain", PLAIN), ("ldx", LDX), ("ldr", LDR), ("window", WINDOW), ("res1", RES1),
             ("res2", dict(RES2, H=8, W=12), _to_direct(refused_forced="f43")),      # (an upsampled residual needs even Ho, Wo)
             ("relu1", RELU1), ("relu2", RELU2), ("nobias", NOBIAS),
             ("cstride2", CSTRIDE2, _to_direct(refused_forced="f43")), ("all1", ALL1), ("n0", N0)]
_FULL = dict(routing=(("ragged", False),))
# narrow: 32 tiles x 64 channels, k-tiles of 16: 16 -> 64 on 4 x 9 x 11 (36 tiles: 2 blocks, the last ragged; odd sizes), one
# k-tile, and 32 -> 64 (2 k-tiles); wide: 16 tiles x 128 channels, k-tiles of 32: 32 -> 128 and 64 -> 128 on 2 x 9 x 11 (18 tiles)
_rows("f43-narrow", dict(N=4, H=9, W=11, Cin=32, Cout=64, **_FULL), _F43, dict(path="winograd43", entry=W43), _F43_ROWS)
_rows("f43-wide", dict(N=2, H=9, W=11, Cin=64, Cout=128, **_FULL), _F43, dict(path="winograd43", entry=W43), _F43_ROWS)
_rows("f43-1ktile", dict(H=9, W=11, **_FULL), _F43, dict(path="winograd43", entry=W43),
      [("narrow", dict(N=4, Cin=16, Cout=64)), ("wide", dict(N=2, Cin=32, Cout=128))])
# width 4 k + 1 = 5: the ragged entry (paired strip tiles in the same launch; N = 1 and N = 3: an odd image count leaves a half
# pair), predicate glass_winograd43_ragged_supported
_F43R = dict(_F43, predicate="glass_winograd43_ragged_supported", routing=(("ragged", "tiles"),))
_F43R_ROWS = [("plain", PLAIN), ("ldx", LDX), ("ldr", LDR), ("window", WINDOW), ("res1", RES1), ("relu1", RELU1), ("relu2", RELU2),
              ("nobias", NOBIAS), ("all1", ALL1), ("cstride2", CSTRIDE2, _to_direct(refused_forced="f43")),
              ("n0", N0, dict(path="winograd43", entry=W43, predicate=None, exact=False, bound=F43_BOUND))]   # plan_conv: the full form
_rows("f43-ragged-n1", dict(N=1, H=6, W=5, Cin=64, Cout=128), _F43R, dict(path="winograd43r", entry=W43R), _F43R_ROWS)
_rows("f43-ragged-n3", dict(N=3, H=6, W=5, Cin=64, Cout=128), _F43R, dict(path="winograd43r", entry=W43R), _F43R_ROWS)
_rows("f43-ragged-narrow", dict(N=3, H=6, W=5, Cin=32, Cout=64), _F43R, dict(path="winograd43r", entry=W43R),
      [("plain", PLAIN), ("all1", ALL1)])
# ... and the body + strip form (Routing.ragged True): needs dense rows like "f22r"; a wider pixel falls back to the full F(4x4) launch
_F43B = dict(_F43, routing=(("ragged", True),), strip=True)
_F43B_ROWS = [("plain", PLAIN), ("ldx", LDX, dict(path="winograd43", entry=W43, predicate=None, exact=False, bound=F43_BOUND)),
              ("ldr", LDR), ("window", WINDOW), ("res1", RES1), ("relu1", RELU1), ("relu2", RELU2), ("nobias", NOBIAS),
              ("all1", dict(ALL1, ldx_pad=0)), ("cstride2", CSTRIDE2, _to_direct(refused_forced="f43")),
              ("n0", N0, dict(path="winograd43", entry=W43, predicate=None, exact=False, bound=F43_BOUND))]
_rows("f43-body-n1", dict(N=1, H=6, W=5, Cin=64, Cout=128), _F43B, dict(path="winograd43r", entry=W43B), _F43B_ROWS)
_rows("f43-body-n3", dict(N=3, H=6, W=5, Cin=64, Cout=128), _F43B, dict(path="winograd43r", entry=W43B), _F43B_ROWS)
# split-K (wide shape only, slices dividing Cin / 32): f43k = 2 on a 6 x 9 map, (2, body) on 6 x 5; the reducer applies the epilogue
_F43K = dict(fn="conv", KH=3, KW=3, pad=(1, 1), forced=None, predicate="glass_winograd43_splitk_supported", exact=False, bound=F43K_BOUND)
# (refused: the slices stay named for the predicate; the direct kernel, forced, takes the layer)
_F43K_NO = dict(path="direct", entry=D, forced=False, routing=(("splitk", False),))
_F43K_ROWS = [("plain", PLAIN), ("ldr", LDR), ("window", WINDOW), ("res1", RES1), ("relu1", RELU1), ("relu2", RELU2),
              ("nobias", NOBIAS), ("all1", dict(ALL1, ldx_pad=0)),
              ("cstride2", CSTRIDE2, _F43K_NO)]
_rows("f43k-full", dict(N=2, H=6, W=9, Cin=64, Cout=128, f43k=2), _F43K, dict(path="winograd43k", entry=W43K),
      _F43K_ROWS + [("ldx", LDX), ("all1-ldx", ALL1), ("res2", dict(RES2, W=8), _F43K_NO), ("n0", N0)])
_rows("f43k-body", dict(N=3, H=6, W=5, Cin=64, Cout=128, f43k=(2, True)), _F43K, dict(path="winograd43k", entry=W43K, strip=True),
      _F43K_ROWS + [("n0", dict(N0, strip=False))])           # (no body form without pixels)

# ------------------------------------------------------------------------------------------------ 1x1 kernels
# glass_pointwise_supported / glass_pointwise_split_supported: 1x1, pad 0, square stride, Cin % 32, Cout % 128, unit channel
# step, ldx / ldy / y_coff / ldr % 4, res_mode 0/1/2 (2: even Ho, Wo)
_PW = dict(fn="conv", forced=None, routing=(("pw", "all"), ("split", 0), ("splitk", False)), predicate="glass_pointwise_supported")
_PW_OK = dict(path="pointwise", entry=PW)
_PWS = dict(fn="conv", forced="pws9", predicate="glass_pointwise_split_supported")
_PWS_OK = dict(path="pointwise_split", entry=PWS)


def _pw_rows(refusal):
    return [("plain", PLAIN), ("ldx", LDX), ("ldr", LDR), ("window", WINDOW), ("res1", RES1), ("res2", RES2), ("relu1", RELU1),
            ("relu2", RELU2), ("nobias", NOBIAS), ("cstride2", CSTRIDE2, refusal), ("all1", ALL1), ("all2", ALL2), ("n0", N0)] + WIDE


_S2_ROWS = [("plain", PLAIN), ("all1", ALL1), ("ldx", LDX), WIDE[0]]
for _cin in (32, 96):
    # 2 x 6 x 14 = 168 pixels (ragged last block), 1 and 3 k-tiles; stride 2 on an odd 7 x 11 map -> 3 x 4 x 6 = 72 pixels
    _rows(f"pw-cin{_cin}", dict(N=2, H=6, W=14, Cin=_cin, Cout=128), _PW, _PW_OK, _pw_rows(dict(path="direct", entry=D)))
    _rows(f"pw-cin{_cin}-s2", dict(N=3, H=7, W=11, Cin=_cin, Cout=128, stride=(2, 2)), _PW, _PW_OK, _S2_ROWS)
    _rows(f"pws-cin{_cin}", dict(N=2, H=6, W=14, Cin=_cin, Cout=128), _PWS, _PWS_OK, _pw_rows(_to_direct(refused_forced="pws9")))
    _rows(f"pws-cin{_cin}-s2", dict(N=3, H=7, W=11, Cin=_cin, Cout=128, stride=(2, 2)), _PWS, _PWS_OK, _S2_ROWS)
# dual-source bf16-split (conv1x1_dual_nhwc: dense operands, res_mode 0): 32 + 32 -> 128, stride 1 and stride 2 on an odd map
_DUAL = dict(fn="dual", Cin=32, Cin2=32, Cout=128, predicate="glass_pointwise_split_dual_supported")
_DUAL_ROWS = [("plain", PLAIN), ("relu1", dict(relu=1)), ("nobias", NOBIAS), WIDE[0], ("wide-relu1", dict(relu=1, wide=9)), ("n0", N0)]
_rows("dual-s1", dict(N=2, H=6, W=14), _DUAL, _PWS_OK | dict(entry=DUAL), _DUAL_ROWS)
_rows("dual-s2", dict(N=3, H=7, W=11, stride=(2, 2)), _DUAL, _PWS_OK | dict(entry=DUAL), _DUAL_ROWS)

# ------------------------------------------------------------------------------------------------ fp16 modes
# fp32 tensors, precision "fp16": glass_conv2d_nhwc_f16 (the fp32 template with operands rounded to fp16 as they are staged) takes
# every valid descriptor; 3x3 32 -> 64 on 2 x 6 x 14 (Cin % 64 != 0 keeps the packed kernel away)
_F16M = dict(fn="conv", forced=None, routing=(("precision", "fp16"),))
_rows("f16", dict(N=2, H=6, W=14, Cin=32, Cout=64, KH=3, KW=3, pad=(1, 1)), _F16M, dict(path="direct_fp16", entry=F16), _DIRECT_ROWS + WIDE5)
# ... and Cout % 4 != 0: the scalar epilogue (3x3 36 -> 42 on 8 x 18)
_COUT42 = dict(N=1, H=8, W=18, Cin=36, Cout=42, KH=3, KW=3, pad=(1, 1))
_rows("f16-cout42", _COUT42, _F16M, dict(path="direct_fp16", entry=F16), [("plain", PLAIN), ("all1", ALL1), ("all2", ALL2)])
# fp16 storage, precision "fp16s": glass_conv2d_nhwc_h16 with every combination of the three half flags (x, y, residual)
_H16M = dict(fn="conv", forced=None, routing=(("precision", "fp16s"),))
_H16_OK = dict(path="direct_fp16", entry=H16)
_rows("h16", dict(N=2, H=6, W=14, Cin=32, Cout=64, KH=3, KW=3, pad=(1, 1)), _H16M, _H16_OK,
      [(f"flags{f}-{n}", dict(o, half=f)) for f in (1, 2, 3, 4, 5, 6, 7) for n, o in (("all1", ALL1), ("all2", ALL2))] +
      [("flags7-plain", dict(half=7)), ("flags7-cstride2", dict(CSTRIDE2, half=7)), ("flags7-n0", dict(N0, half=7)),
       ("flags3-relu1", dict(RELU1, half=3)), ("flags2-nobias", dict(NOBIAS, half=2))] +
      [(n + "-flags7", dict(o, half=7)) for n, o in WIDE5] + [("wide-flags1", dict(ALL1, half=1, wide=5))] +
      # the scalar epilogue with an fp32 / fp16 residual and an fp32 / fp16 output
      [(f"flags{f}-{n}-cstride2", dict(o, half=f)) for f in (4, 5, 6, 7) for n, o in (("all1", ALL1C), ("all2", ALL2C))])
_rows("h16-cout42", _COUT42, _H16M, _H16_OK,
      [("flags7-plain", dict(half=7)), ("flags7-ldr", dict(LDR, half=7)), ("flags7-res2", dict(RES2, half=7)),
       ("flags7-relu2", dict(RELU2, half=7)), ("flags7-all1", dict(ALL1, half=7)), ("flags7-all2", dict(ALL2, half=7)),
       ("flags5-all1", dict(ALL1, half=5)), ("flags6-all2", dict(ALL2, half=6)), ("flags3-all1", dict(ALL1, half=3))])
# ... the packed fp16-MFMA kernel: fp16 input, Cin % 64, Cout % 64, ldx % 8, unit channel step, 16-byte output / residual granules
_H16P = dict(fn="conv", forced=None, routing=(("precision", "fp16s"),), predicate="glass_conv_h16_supported")
_H16P_OK = dict(path="packed_fp16", entry=H16P)
_H16P_ROWS = [("plain", PLAIN), ("ldx", LDX), ("ldr", LDR), ("window", WINDOW), ("res1", RES1), ("res2", RES2), ("relu1", RELU1),
              ("relu2", RELU2), ("nobias", NOBIAS), ("cstride2", CSTRIDE2, _H16_OK), ("all1", ALL1), ("all2", ALL2), ("n0", N0),
              ("all1-cstride2", ALL1C, _H16_OK)] + WIDE5
_rows("h16p-64-flags7", dict(N=2, H=6, W=14, Cin=64, Cout=64, KH=3, KW=3, pad=(1, 1), half=7), _H16P, _H16P_OK, _H16P_ROWS)
_rows("h16p-128-flags7", dict(N=2, H=6, W=14, Cin=128, Cout=128, KH=3, KW=3, pad=(1, 1), half=7), _H16P, _H16P_OK,
      [("plain", PLAIN), ("all1", ALL1), ("all2", ALL2)])
_rows("h16p-flags", dict(N=2, H=6, W=14, Cin=64, Cout=64, KH=3, KW=3, pad=(1, 1)), _H16P, _H16P_OK,
      [(f"flags{f}-{n}", dict(o, half=f)) for f in (1, 3, 5) for n, o in (("all1", ALL1), ("all2", ALL2))] +
      [("s2-flags7", dict(ALL1, half=7, stride=(2, 2), H=7, W=11)), ("1x1-flags7", dict(ALL2, half=7, KH=1, KW=1, pad=(0, 0)))])
# ... and on the cast path: fp32 input rounded to fp16 once (glass_cast_f32_to_f16), KH KW Cout = 576 >= 512
_rows("h16p-cast", dict(N=2, H=6, W=14, Cin=64, Cout=64, KH=3, KW=3, pad=(1, 1)), dict(_H16P, routing=(("precision", "fp16"),)),
      _H16P_OK, [("plain", PLAIN), ("ldx", LDX), ("all1", ALL1), ("all2", ALL2), WIDE5[1],
                 ("fp16s", dict(ALL1, routing=(("precision", "fp16s"),))),
                 ("n0", N0, dict(path="direct_fp16", entry=F16, predicate=None))])        # nothing to cast: the template returns at once

# ------------------------------------------------------------------------------------------------ linear
# x [M,K] @ w [11,K]^T on the implicit-GEMM kernel (128 x 32 tiles, Cout % 4 != 0: the scalar epilogue); plain and split-K
_LIN = dict(fn="linear", Cout=11, H=1, W=1, forced=None)
_LIN_ROWS = [("plain", PLAIN), ("relu1", dict(relu=1)), ("nobias", NOBIAS), ("wide-out", dict(ldy_tail=5)), ("m0", N0)]
_rows("linear-k64", dict(N=5, Cin=64, routing=(("splitk", False),)), _LIN, _DIRECT_OK, _LIN_ROWS)
_rows("linear-k192", dict(N=130, Cin=192, routing=(("splitk", False),)), _LIN, _DIRECT_OK, _LIN_ROWS)
_LINK = dict(_LIN, slices=4, predicate="glass_conv2d_splitk_supported")
_LINK_ROWS = _LIN_ROWS[:4] + [("m0", N0, dict(path="direct", entry=D))]
_rows("linear-splitk-k512", dict(N=5, Cin=512), _LINK, _SPLITK_OK, _LINK_ROWS)
_rows("linear-splitk-k256-m130", dict(N=130, Cin=256, slices=2), _LINK, _SPLITK_OK, _LINK_ROWS)

# ------------------------------------------------------------------------------------------------ fused stems
# glass_backbone_stem_supported: H, W multiples of 4 (N counts images); glass_local_stem_supported: multiples of 32 (N counts crops)
_rows("backbone-stem", dict(fn="backbone_stem", Cin=4, Cout=64, path="fused_stem", entry=BSTEM, predicate="glass_backbone_stem_supported"),
      {}, {}, [("4x4", dict(N=1, H=4, W=4)), ("2x36x44", dict(N=2, H=36, W=44)),
               ("38x44", dict(N=1, H=38, W=44), dict(path="direct", entry=D))])     # refused: conv2d_nhwc + maxpool2d_nhwc instead
_rows("local-stem", dict(fn="local_stem", Cin=4, Cout=32, path="local_stem", entry=LSTEM, predicate="glass_local_stem_supported"),
      {}, {}, [("32x32", dict(N=1, H=32, W=32)), ("3x32x64", dict(N=3, H=32, W=64)), ("n0", dict(N=0, H=32, W=32)),
               ("32x48", dict(N=1, H=32, W=48), dict(path="direct", entry=D))])     # refused: the three separate launches

# the number of rows each route must have (literals: a route cannot lose rows without this table changing too)
ROUTE_ROWS = {
    "direct-128x32": 15, "direct-stem7x7": 15, "direct-cin36-cout40": 15, "direct-cin36-cout42": 15, "direct-2x2s21": 15,
    "direct-2x1s21": 15, "direct-128x96": 15, "direct-k256-64x64": 15, "direct-fewtile-64x64": 15, "direct-64x128": 15,
    "direct-128x128": 4, "splitk-64x64": 13, "splitk-128x32": 13,
    "f22-64": 12, "f22-128": 12, "f22-1x3x5": 4, "f22r-64": 11, "f22r-128": 11,
    "f43-narrow": 12, "f43-wide": 12, "f43-1ktile": 2, "f43-ragged-n1": 11, "f43-ragged-n3": 11, "f43-ragged-narrow": 2,
    "f43-body-n1": 11, "f43-body-n3": 11, "f43k-full": 13, "f43k-body": 10,
    "pw-cin32": 16, "pw-cin32-s2": 4, "pws-cin32": 16, "pws-cin32-s2": 4,
    "pw-cin96": 16, "pw-cin96-s2": 4, "pws-cin96": 16, "pws-cin96-s2": 4,
    "dual-s1": 6, "dual-s2": 6,
    "f16": 18, "f16-cout42": 3, "h16": 31, "h16-cout42": 9, "h16p-64-flags7": 17, "h16p-128-flags7": 3, "h16p-flags": 8, "h16p-cast": 7,
    "linear-k64": 5, "linear-k192": 5, "linear-splitk-k512": 5, "linear-splitk-k256-m130": 5,
    "backbone-stem": 3, "local-stem": 4,
}

BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES), "duplicate case ids"


# ================================================================================================ the library's side of a row
def routing_of(case):
    from glass_amd.ops import native as K
    return K.Routing(**dict(BASE_ROUTING, **dict(case.routing)))


def desc_of(case):
    from glass_amd.ops import native as K
    return K.ConvDesc(*case.desc_ints())


def dtypes_of(case):
    """(x, out, residual) storage dtypes as torch dtypes; residual None without one"""
    import torch
    f = lambda bit: torch.float16 if case.half & bit else torch.float32
    return f(1), f(2), (f(4) if case.res_mode else None)


class forced_slices:
    """the `_splitk_slices` substitution of tests/test_gpu_f_ops.py (test_conv_splitk_matches_the_single_slice_kernel): the row's
    slice count instead of the cost model's"""

    def __init__(self, case):
        self.n = case.slices

    def __enter__(self):
        from glass_amd.ops import native as K
        self.rule = K._splitk_slices
        if self.n is not None:
            n = self.n
            K._splitk_slices = lambda *a, **k: n
        return self

    def __exit__(self, *exc):
        from glass_amd.ops import native as K
        K._splitk_slices = self.rule
        return False


def plan_of(case, forced="row"):
    """ops.native.plan_conv for the row's descriptor, routing and forcing (raw weights: packs None)"""
    from glass_amd.ops import native as K
    xd, od, rd = dtypes_of(case)
    with forced_slices(case):
        return K.plan_conv(desc_of(case), routing_of(case), x_dtype=xd, out_dtype=od, res_dtype=rd, res_mode=case.res_mode, packs=None,
                           forced=case.forced if forced == "row" else forced, f43k=case.f43k)


def predicate_of(case):
    """the verdict of the row's *_supported() on the row's descriptor (host-only library queries), or None without a predicate"""
    import ctypes
    from glass_amd._lib import lib
    if case.predicate is None:
        return None
    fn = getattr(lib(), case.predicate)
    if case.fn in ("backbone_stem", "local_stem"):
        return bool(fn(case.H, case.W))
    d = desc_of(case)
    if case.predicate in ("glass_conv2d_splitk_supported", "glass_winograd43_splitk_supported"):
        return bool(fn(ctypes.byref(d), int(case.slices if case.slices is not None else
                                            (case.f43k[0] if isinstance(case.f43k, tuple) else case.f43k))))
    if case.predicate == "glass_conv_h16_supported":
        return bool(fn(ctypes.byref(d), case.half if case.half else 1))     # (fp32 tensors, the cast path: asked with flags = 1)
    if case.predicate == "glass_pointwise_split_dual_supported":
        return bool(fn(ctypes.byref(d), case.Cin2, case.Cin2))
    return bool(fn(ctypes.byref(d)))
