"""Shared inputs of the feature-exchange tests (tests/test_exchange_host_cpu.py, tests/test_gpu_exchange.py): blocks of 32
float32 values -- one MX block each -- from a seeded generator, and the named edge blocks of the wire format's contract
(include/disconet_hip.h, "Feature exchange wire format").  Everything is numpy; nothing here touches the GPU."""
import numpy as np

BLOCK = 32
F32 = np.float32


def _f(bits):
    return np.array(bits, dtype=np.uint32).view(F32)


def _below(x):
    """the float32 just below |x| in magnitude"""
    return np.nextafter(F32(x), F32(0))


def _above(x):
    return np.nextafter(F32(x), F32(np.inf))


def random_blocks(n_blocks, signed, seed):
    """[n_blocks, 32] float32: uniform [0, 1) times a binade of the block's own from 2^-30 to 2^30 (non-negative, as after
    a ReLU, a tenth of the values exactly 0), or the same with random signs"""
    rng = np.random.RandomState(seed)
    x = rng.rand(n_blocks, BLOCK).astype(F32) * np.exp2(rng.randint(-30, 31, size=(n_blocks, 1))).astype(F32)
    x[rng.rand(n_blocks, BLOCK) < 0.1] = 0
    if signed:
        x = x * np.where(rng.rand(n_blocks, BLOCK) < 0.5, -1, 1).astype(F32)
    return x.astype(F32)


def _block(values, fill=0.0):
    """a block that begins with `values`, the rest `fill`"""
    b = np.full(BLOCK, fill, F32)
    b[:len(values)] = np.array(values, F32)
    return b


def _ties(mant_bits, kmin, emax, e, sign=1):
    """a block whose maximum is 2^(emax + e) exactly (scale exponent e) and whose other values are exact rounding ties
    of the element format under that scale: midpoints of neighbouring codes in the lowest normal binades (even and odd
    lower neighbours), in the subnormal range, half the smallest subnormal (ties to zero) and its two float32 neighbours"""
    q = 2.0 ** (kmin - mant_bits)                          # the subnormal quantum of the element format
    scaled = [2.0 ** emax]
    for k in (kmin, kmin + 1):                             # normal binades: midpoints (j + 0.5) quanta above 2^k
        for j in range(2 ** mant_bits):
            scaled.append(2.0 ** k * (1 + (j + 0.5) / 2 ** mant_bits))
    for j in range(2 ** mant_bits):                        # subnormal range: (j + 0.5) q; j = 0 is half the smallest subnormal
        scaled.append((j + 0.5) * q)
    vals = [F32(s * 2.0 ** e) for s in scaled]
    half = F32(0.5 * q * 2.0 ** e)
    vals += [_below(half), _above(half)]
    assert len(vals) <= BLOCK
    return _block(vals) * F32(sign)


def edge_blocks():
    """name -> [32] float32, in a fixed order"""
    rng = np.random.RandomState(7)
    e = {}
    e["zeros"] = _block([])
    e["neg_zero"] = _block([-0.0, 1.0, -0.0, -1e-10, 1e-10, -0.75])         # -0, and negatives that round to zero
    e["neg_zero_only"] = _block([-0.0, 0.0, -0.0])
    e["subnormals"] = (rng.randint(1, 1 << 23, size=BLOCK).astype(np.uint32) |
                       (rng.randint(0, 2, size=BLOCK).astype(np.uint32) << 31)).view(F32)
    e["subnormal_small"] = _block(_f([1, 2, 3, 0x80000001, 5, 7]))
    e["pow2_max"] = _block([4.0, 3.9, 0.1, 2.0, 1.0, 0.5, 0.25, 0.2, -4.0])
    e["pow2_max_small"] = _block([2.0 ** -100, 2.0 ** -101, 1.7 * 2.0 ** -103, 2.0 ** -110])
    e["clamp"] = _block([_below(512.0), 448.0, 449.0, 463.9, 464.0, 479.0, 480.0, 5.0, 6.0, 7.0, -_below(512.0)])
    e["clamp_fp4"] = _block([_below(8.0), 6.0, 6.9, 7.0, 7.1, 5.0, 5.1, -_below(8.0)])
    e["ties_fp8"] = _ties(3, -6, 8, 0)
    e["ties_fp8_scaled"] = _ties(3, -6, 8, -17)
    e["ties_fp8_negative"] = _ties(3, -6, 8, 3, sign=-1)
    e["ties_fp4"] = _ties(1, 0, 2, 0)
    e["ties_fp4_scaled"] = _ties(1, 0, 2, 11)
    e["ties_fp4_negative"] = _ties(1, 0, 2, -5, sign=-1)
    e["ties_lowest_scale"] = _ties(3, -6, 8, -127)                # e = -127: the element quanta are fp32 subnormals
    e["one_nan"] = _block([1.0, 2.0, np.nan, -3.0], fill=0.5)
    e["plus_inf"] = _block([1.0, np.inf, -3.0], fill=0.5)
    e["minus_inf"] = _block([1.0, -np.inf, -3.0], fill=0.5)
    e["huge"] = _block([3.0e38, -3.0e38, 1.0e38, 1.0, 3.4028235e38])
    e["huge_alone"] = _block([3.0e38])
    e["tiny"] = _block([1e-45, -1e-45, 0.0])
    e["tiny_beside_one"] = _block([1e-45, 1.0, -1e-45])
    # binary16 edges: the largest finite value, the rounding boundary to Inf, and the subnormal ties (quantum 2^-24)
    q16 = 2.0 ** -24
    e["f16_edges"] = _block([65504.0, 65519.99, 65520.0, -65519.99, -65520.0, 0.5 * q16, _below(0.5 * q16), _above(0.5 * q16),
                             1.5 * q16, 2.5 * q16, -0.5 * q16, -1.5 * q16, 1023.5 * q16, 1024.5 * q16, 2.0 ** -14,
                             _below(2.0 ** -14), 1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11])
    for b in e.values():
        assert b.shape == (BLOCK,) and b.dtype == F32
    return e


def edge_array():
    """every edge block stacked: [n_edges, 32] float32"""
    return np.stack(list(edge_blocks().values()))


def tensor_with_edges(n, h, w, c, seed, signed=True):
    """An [n, h, w, c] float32 tensor of random blocks with the edge blocks placed where a kernel's indexing can go
    wrong: from the first block of the first pixel on, ending at the last block of the last pixel, across wave
    boundaries (a wave holds 16 blocks) where the image is that long, and at the start of the last image.  Small tensors
    take as many edge blocks as fit."""
    per_image = h * w * c // BLOCK
    x = random_blocks(n * per_image, signed, seed).reshape(n, per_image, BLOCK)
    edges = edge_array()
    k = len(edges)

    def put(image, first):
        first = max(0, min(first, per_image - 1))
        m = min(k, per_image - first)
        x[image, first:first + m] = edges[:m]

    put(0, 26)                                   # across the boundaries of waves 1 | 2 and 2 | 3 (blocks 32 and 48)
    put(0, 0)                                    # the first pixel, on across the boundary of waves 0 | 1 (block 16)
    put(n - 1, per_image - k)                    # ... through the last block of the last pixel of the last image
    if n > 1:
        put(n - 1, 0)
        x[0, per_image - 1] = edges[min(k - 1, 10)]
    return x.reshape(n, h, w, c)
