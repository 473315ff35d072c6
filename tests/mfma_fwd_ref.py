"""CPU references of the matrix-core forward tables (mfma_fwd_rows.py): the three-way bf16 split of csrc/conv1x1_x3.hip and the weight
image idiff_pack_conv1x1_x3 writes, the weight image of idiff_pack_conv_weight_bf16, the rounding contract of csrc/conv_bf16.hip, and
the integer operands of the exact rows.  Plain torch on the CPU; nothing here imports the library."""
import torch
import torch.nn.functional as F

from conv_branch_ref import make_inputs, silu  # noqa: F401
from conv_branch_rows import N, S, U, out_size
from mfma_fwd_rows import BM, CKB, cin


# ---- bf16x3: x = p1 + p2 + p3, each the upper 16 bits of an fp32 value ----------------------------------------------------------------
def hi16(x):
    """an fp32 tensor with the lower 16 bits of every element cleared (truncation to bf16, kept in fp32)"""
    assert x.dtype == torch.float32
    return (x.contiguous().view(torch.int32) & -65536).view(torch.float32)


def split3(x):
    """p1 = hi16(x), p2 = hi16(x - p1), p3 = hi16(x - p1 - p2): both subtractions are exact in fp32"""
    p1 = hi16(x)
    r1 = x - p1
    p2 = hi16(r1)
    p3 = hi16(r1 - p2)
    return p1, p2, p3


def bf16_bits(x):
    """the upper halves of an fp32 tensor as int16"""
    return (x.contiguous().view(torch.int32) >> 16).to(torch.int16)


def x3_image(w):
    """idiff_pack_conv1x1_x3 of w [Cout, Cin]: int16 [chunk of 32 ci][block of 64 co][plane 3][octet 4][co 64][8], zero beyond w"""
    Cout, Cin = w.shape
    ncob, ncc = -(-Cout // BM), -(-Cin // CKB)
    wp = torch.zeros(ncob * BM, ncc * CKB, dtype=torch.float32)
    wp[:Cout, :Cin] = w
    planes = torch.stack([bf16_bits(p) for p in split3(wp)])  # [plane][co][ci]
    return planes.view(3, ncob, BM, ncc, 4, 8).permute(3, 1, 0, 4, 2, 5).contiguous().view(-1)


def rne_bits(x):
    """fp32 -> bf16 (round to nearest even) as int16"""
    return x.float().to(torch.bfloat16).view(torch.int16)


def conv_weight(w, transpose):
    """the conv's weight [Cout', Cin', 3, 3] of a stored weight packed with `transpose` (the data gradient: in/out swapped, taps
    flipped)"""
    return w.permute(1, 0, 2, 3).flip(2, 3).contiguous() if transpose else w


def bf16_image(w, transpose=False):
    """idiff_pack_conv_weight_bf16 of the stored 3x3 weight w: int16 [chunk of 32 ci][block of 64 co][tap 9][octet 4][co 64][8]"""
    wc = conv_weight(w, transpose)
    Cc, Kc = wc.shape[:2]
    ncob, nck = -(-Cc // BM), -(-Kc // CKB)
    wp = torch.zeros(ncob * BM, nck * CKB, 9, dtype=torch.float32)
    wp[:Cc, :Kc] = wc.reshape(Cc, Kc, 9)
    return rne_bits(wp).view(ncob, BM, nck, 4, 8, 9).permute(2, 0, 5, 3, 1, 4).contiguous().view(-1)


def stored_weight(row, inp):
    """the weight tensor handed to pack_conv_weight(transpose=row['transposed']) so that the conv's weight is inp['w']"""
    w = inp["w"]
    if not row["transposed"]:
        return w
    return w.permute(1, 0, 2, 3).flip(2, 3).contiguous()


# ---- bf16 operands: the rounding contract ---------------------------------------------------------------------------------------------
def rne_bf16(t):
    """fp32 -> bf16 (round to nearest even) -> float64"""
    return t.float().to(torch.bfloat16).double()


def gathered(row, inp, dtype):
    """the conv's input operand in `dtype`: prologue silu(a*x+b) on src0, virtual concat, nearest x2 upsample / pixel-unshuffle"""
    x = inp["src0"].to(dtype)
    if inp["pro"] is not None:
        pa, pb = (t.to(dtype)[:, :, None, None] for t in inp["pro"])
        x = F.silu(pa * x + pb) if dtype == torch.float32 else silu(pa * x + pb)
    if inp["src1"] is not None:
        x = torch.cat([x, inp["src1"].to(dtype)], 1)
    if row["mode"] == U:
        x = x.repeat_interleave(2, 2).repeat_interleave(2, 3)
    elif row["mode"] == S:
        x = F.pixel_unshuffle(x, 2)
    return x


def conv64(x, w):
    return F.conv2d(x.double(), w.double(), padding=w.shape[-1] // 2)


def epilogue64(row, inp):
    """(bias, rest): what the fp32 epilogue adds to the sum, in fp64 -- the bias (part of the statistics) and vec + res + silu(aux)"""
    Hout, Wout = out_size(row)
    z = torch.zeros(row["B"], row["Cout"], Hout, Wout, dtype=torch.float64)
    bias = z if inp["bias"] is None else z + inp["bias"].double()[None, :, None, None]
    rest = z
    if inp["vec"] is not None:
        rest = rest + inp["vec"].double()[:, :, None, None]
    if inp["res"] is not None:
        rest = rest + inp["res"].double()
    if inp["aux"] is not None:
        t, aa, ab = (v.double() for v in inp["aux"])
        rest = rest + silu(aa[:, :, None, None] * t + ab[:, :, None, None])
    return bias, rest


def bf16_references(row, inp):
    """dict of the fp64 tensors the contract is stated in: ref_f64 (unrounded), ref_bf16 (operands gathered in fp32 and rounded once,
    as the kernel does), absconv / absconv_bf16 = conv(|X|, |W|) of either, raw_bf16 = conv + bias of the rounded operands"""
    w = inp["w"]
    x64, x32 = gathered(row, inp, torch.float64), gathered(row, inp, torch.float32)
    xr, wr = rne_bf16(x32), rne_bf16(w)
    bias, rest = epilogue64(row, inp)
    return dict(ref_f64=conv64(x64, w) + bias + rest, ref_bf16=conv64(xr, wr) + bias + rest, absconv=conv64(x64.abs(), w.abs()),
                absconv_bf16=conv64(xr.abs(), wr.abs()), raw_bf16=conv64(xr, wr) + bias)


def contract_bound(row, refs):
    """(reference, elementwise bound) of a bf16 row.  Without a prologue the operands are exact copies, their rounding is deterministic:
    |got - ref_bf16| <= 5e-5 conv(|X~|,|W~|) + 4e-7 |ref_bf16| (test_conv_bf16_gpu._contract_checks).  With one, silu_fast and the CPU's
    fp32 SiLU may differ in the last bit and flip a rounding, so the bound is the rigorous one from the unrounded reference: each
    operand and each weight is rounded once, at most 2^-9 relative each: |got - ref_f64| <= 2^-8 conv(|X|,|W|) + 4e-7 |ref_f64|."""
    if row["pro"]:
        return refs["ref_f64"], 2.0 ** -8 * refs["absconv"] + 4e-7 * refs["ref_f64"].abs() + 1e-30
    return refs["ref_bf16"], 5e-5 * refs["absconv_bf16"] + 4e-7 * refs["ref_bf16"].abs() + 1e-30


def rms(t):
    return float(t.double().pow(2).mean().sqrt())


# ---- exact rows -----------------------------------------------------------------------------------------------------------------------
def int_inputs(row, seed):
    """make_inputs with every operand an integer in [-2, 2] (no prologue, no aux term): each value is its own first bf16 plane, every
    product and every partial sum is exact in fp32 (|sum| <= 4 Cin ks^2 + 6)"""
    assert not row["pro"] and not row["aux"]
    g = torch.Generator().manual_seed(seed)
    B, C0, C1, Cout, Hin, Win, ks = (row[k] for k in ("B", "C0", "C1", "Cout", "Hin", "Win", "ks"))
    Hout, Wout = out_size(row)

    def ints(*shape):
        return torch.randint(-2, 3, shape, generator=g).float()

    inp = dict(src0=ints(B, C0, Hin, Win), src1=ints(B, C1, Hin, Win) if C1 else None, w=ints(Cout, cin(row), ks, ks),
               bias=ints(Cout) if row["bias"] else None, pro=None, res=ints(B, Cout, Hout, Wout) if row["res"] else None,
               vec=ints(B, Cout) if row["vec"] else None, aux=None)
    assert row["mode"] in (N, U, S)
    return inp
