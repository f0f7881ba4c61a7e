"""Independent references for the delta-codec tests.

e4m3 (OCP fp8 e4m3fn) is built here from the format definition alone: one
sign bit, four exponent bits with bias 7, three mantissa bits; exponent 0
holds the subnormals man * 2^-9; exponent 15 with mantissa 7 is NaN, there
are no infinities, and the largest value is 1.75 * 2^8 = 448.  The encoder
is nearest-value with ties to the even code, clamped at +-448, NaN to 0x7F.
Nothing here uses torch.float8_e4m3fn or the project's own converters: the
point of this file is to disagree with them if they are wrong.

All arithmetic is fp64 on fp32 inputs.  The tie decision compares 2|x| with
the sum of the two neighbouring code values, both exact in fp64.
"""
import numpy as np
import torch


def e4m3_table() -> np.ndarray:
    """fp64 value of each of the 256 codes (NaN at 0x7F and 0xFF)."""
    out = np.empty(256, dtype=np.float64)
    for code in range(256):
        exp, man = (code >> 3) & 0xF, code & 7
        if exp == 0xF and man == 7:
            v = float("nan")
        elif exp == 0:
            v = man * 2.0 ** -9
        else:
            v = (1.0 + man / 8.0) * 2.0 ** (exp - 7)
        out[code] = -v if code & 0x80 else v
    return out


E4M3 = e4m3_table()
E4M3_POS = E4M3[:0x7F].copy()          # codes 0x00..0x7E, strictly increasing
E4M3_MAX = 448.0
assert E4M3_POS[-1] == E4M3_MAX and np.all(np.diff(E4M3_POS) > 0)


def e4m3_midpoints() -> np.ndarray:
    """The 126 midpoints between adjacent non-negative codes; every one is an
    fp32 (indeed bf16) number."""
    return (E4M3_POS[:-1] + E4M3_POS[1:]) / 2.0


def e4m3_encode(x) -> np.ndarray:
    """uint8 code of each element of x (any float array or tensor)."""
    if isinstance(x, torch.Tensor):
        x = x.detach().cpu().double().numpy()
    x = np.asarray(x, dtype=np.float64)
    a = np.minimum(np.abs(x), E4M3_MAX)
    a = np.where(np.isnan(a), 0.0, a)
    hi = np.clip(np.searchsorted(E4M3_POS, a, side="left"), 0, 0x7E)
    lo = np.clip(hi - 1, 0, 0x7E)
    two_a = 2.0 * a
    mid2 = E4M3_POS[lo] + E4M3_POS[hi]
    even = np.where(lo % 2 == 0, lo, hi)
    code = np.where(two_a > mid2, hi, np.where(two_a < mid2, lo, even))
    code = code.astype(np.uint8) | np.where(np.signbit(x), 0x80, 0).astype(np.uint8)
    return np.where(np.isnan(x), np.uint8(0x7F), code).astype(np.uint8)


def e4m3_decode(codes) -> np.ndarray:
    return E4M3[np.asarray(codes, dtype=np.uint8)]


# ------------------------------------------------------------ bf16 helpers

def bf16_rne(t: torch.Tensor) -> torch.Tensor:
    """Round-to-nearest-even to bf16 (torch's own conversion)."""
    return t.to(torch.bfloat16)


def bits16(t: torch.Tensor) -> torch.Tensor:
    return t.contiguous().view(torch.int16)


def bits32(t: torch.Tensor) -> torch.Tensor:
    return t.contiguous().view(torch.int32)


def f32_nextafter(x, toward):
    return np.nextafter(np.asarray(x, dtype=np.float32),
                        np.float32(toward)).astype(np.float32)


def with_neighbours(vals) -> np.ndarray:
    """Each fp32 value followed by its fp32 neighbours above and below."""
    v = np.asarray(vals, dtype=np.float32)
    return np.concatenate([v, f32_nextafter(v, np.inf),
                           f32_nextafter(v, -np.inf)]).astype(np.float32)


# ------------------------------------------------------- table test inputs

CROSSING = [262145, 7, 64, 300001, 1, 129]   # padded total > 2048 * 256
SIZE_LISTS = {
    "two64": [64, 64],
    "ones": [1, 1, 1],
    "mixed": [100, 64, 4096, 1],
    "odd": [63, 65, 127, 129, 2],
    "crossing": CROSSING,
}
ALL_LISTS = dict(SIZE_LISTS, k1000=[1000])
SAMPLED_LISTS = ["k1000", "mixed", "crossing"]
SAMPLED_STRIDES = [1, 2, 7, 64, 65]
MAGS = {"down": -2, "up": 2}                 # tensor t scaled by 10^(+-2t)
POW2_STANDOFF = 1e-6


def table_parts(name, mag, bf16, seed_bump=0):
    """Per-tensor fp32 CPU residuals of a size list; bf16-representable when
    `bf16`.  Neighbouring tensors differ by 100x, so a value leaking across
    a tensor boundary moves that tensor's power-of-two scale."""
    sizes = ALL_LISTS[name]
    seed = (1000 * sorted(ALL_LISTS).index(name) + 10 * sorted(MAGS).index(mag)
            + int(bf16) + 100000 * seed_bump)
    g = torch.Generator().manual_seed(seed)
    parts = [torch.randn(s, generator=g) * 10.0 ** (MAGS[mag] * t)
             for t, s in enumerate(sizes)]
    if bf16:
        parts = [p.to(torch.bfloat16).float() for p in parts]
    return parts


def rms64(x, stride=1) -> float:
    """fp64 RMS over x[::stride] (count ceil(n / stride))."""
    s = np.asarray(x, dtype=np.float64)[::stride]
    return float(np.sqrt(np.sum(s * s) / max(s.size, 1)))


def pow2_distance(x: float) -> float:
    """Relative distance of x > 0 from the nearest power of two."""
    if not x > 0:
        return float("inf")
    m, _ = np.frexp(x)                        # m in [0.5, 1)
    return float(min(m - 0.5, 1.0 - m) / m)


def assert_rms_standoff(x, stride=1, what=""):
    """A condition on the inputs, not a tolerance on the kernel: the 1-bit
    statistic is a double sum added atomically in no fixed order, so its
    last bits vary; the power-of-two floor of the RMS is order-independent
    as long as the RMS is not within rounding of a power of two."""
    r = rms64(x, stride)
    if r == 0.0:
        return
    d = pow2_distance(r)
    assert d >= POW2_STANDOFF, (
        f"input {what}: RMS {r!r} is {d:.2e} (relative) from a power of two; "
        f"pick another seed")
