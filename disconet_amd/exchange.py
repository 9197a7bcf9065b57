"""The feature-exchange wire format: what an agent sends the others in 16, 8.25 or 4.25 bits per value.

include/disconet_hip.h ("Feature exchange wire format") is the contract; host_encode / host_decode state it again in
numpy -- integer operations on the fp32 bit patterns, no float8 type anywhere -- and the kernels of csrc/exchange.hip
(ops.exchange_encode / exchange_decode) equal them in every byte.  roundtrip() is what a receiver sees of a sender's map.

    message of one [h, w, c] image = payload | scale bytes | zeros up to a multiple of 16
    f16    2 bytes per value (numpy.astype(float16)), no scales
    mxfp8  1 byte per value (E4M3), one E8M0 scale byte per 32 channels of a pixel
    mxfp4  two values per byte (E2M1, the lower channel in the low nibble), the same scales

Selective exchange (the header's "Selective exchange", csrc/exchange_cells.hip): an agent sends the K strongest cells of
its map, in any of the four formats.  host_select / host_encode_cells / host_decode_cells state it in numpy.

    score of a cell = max over its channels of (bits & 0x7fffffff); the selected cells are the first min(K, non-zero cells)
    by (score descending, index ascending), listed in ascending index
    message of one image = uint32 count + 12 zero bytes | K uint16 indices (0xFFFF beyond count), zeros up to a multiple
    of 16 | the dense message of the gathered [1, K, c] image (rows beyond count are +0.0)
"""
import numpy as np

from . import ops
from .ops import EXCHANGE_FORMATS as FORMATS               # name -> DN_EXCHANGE_*

BLOCK = 32                                                  # channels that share a scale

# element formats: mantissa bits, exponent of the smallest normal binade, largest magnitude code, emax, sign bit
_ELEM = {"mxfp8": (3, -6, 0x7E, 8, 0x80), "mxfp4": (1, 0, 0x7, 2, 0x8)}


def check_format(fmt):
    if fmt not in FORMATS:
        raise ValueError("exchange format must be one of %s (got %r)" % (" | ".join(FORMATS), fmt))
    return fmt


def _layout(fmt, h, w, c):
    """(payload bytes, scale bytes, message bytes) of one [h, w, c] image"""
    check_format(fmt)
    if min(h, w, c) <= 0 or c % BLOCK:
        raise ValueError("exchange: a %d x %d x %d map: the channel count must be a positive multiple of %d" % (h, w, c, BLOCK))
    values = h * w * c
    payload = {"f32": 4 * values, "f16": 2 * values, "mxfp8": values, "mxfp4": values // 2}[fmt]
    scales = values // BLOCK if fmt in _ELEM else 0
    return payload, scales, payload + (scales + 15) // 16 * 16


def message_bytes(fmt, h, w, c):
    """bytes one agent sends per frame for an [h, w, c] map (dn_exchange_message_bytes)"""
    return _layout(fmt, h, w, c)[2]


def scale_offset(fmt, h, w, c):
    """where the scale bytes begin inside a message (= the payload's length)"""
    return _layout(fmt, h, w, c)[0]


def _block_scale(bits, emax):
    """bits [blocks, 32] uint32 -> (scale exponent e [blocks] int64, non-finite flag [blocks])"""
    m = (bits & np.uint32(0x7fffffff)).max(axis=1).astype(np.int64)      # fp32 magnitudes order as their bit patterns
    bad = m >= 0x7f800000
    # E = biased exponent - 127; a subnormal or zero maximum (exponent field 0) lies below -127 + emax and clamps to -127
    e = np.maximum((m >> 23) - 127 - emax, -127)
    return e, bad


def _elem_codes(bits, e, fmt):
    """the element codes of bits [blocks, 32] under the scale exponents e [blocks]: v * 2^-e rounded to nearest even as
    an integer count of the format's quantum, never formed as a float"""
    mb, kmin, max_code, _, sign = _ELEM[fmt]
    a = (bits & np.uint32(0x7fffffff)).astype(np.int64)
    ev = a >> 23
    x = np.maximum(ev, 1)                                   # |v| = M * 2^(x - 150)
    M = (a & 0x7fffff) | np.where(ev > 0, 0x800000, 0)
    p = np.zeros_like(M)                                    # msb(M) (0 for M == 0)
    for s in (16, 8, 4, 2, 1):
        big = (M >> (p + s)) > 0
        p = np.where(big, p + s, p)
    kk = p + x - 150 - e[:, None] - kmin                    # binade of the scaled element, above the smallest normal one
    sh = np.minimum(p - mb - np.minimum(kk, 0), 40)         # right shift to the quantum (>= 13; >= 25 gives 0)
    half = (np.int64(1) << (sh - 1)) - 1
    R = (M + half + ((M >> sh) & 1)) >> sh
    code = np.minimum(R + (np.maximum(kk, 0) << mb), max_code)
    return (code | np.where(bits >> np.uint32(31), sign, 0)).astype(np.uint8)


def _elem_values(code, e, fmt):
    """value(code) * 2^e as float32 (exact: see the header), code [blocks, 32] uint8, e [blocks]"""
    mb, kmin, _, _, sign = _ELEM[fmt]
    mag = code.astype(np.int64) & (sign - 1)
    eb = mag >> mb
    mant = mag & ((1 << mb) - 1)
    integer = np.where(eb > 0, mant | (1 << mb), mant)
    v = np.ldexp(integer.astype(np.float64), np.maximum(eb, 1) - 1 + kmin - mb + e[:, None]).astype(np.float32)
    if fmt == "mxfp8":
        v = np.where(mag == 0x7F, np.float32(np.nan), v)
    return np.where((code & sign) != 0, -v, v).astype(np.float32)


def host_encode(feat, fmt):
    """feat [n, h, w, c] float32 (numpy, or anything numpy.asarray takes) -> wire [n, message_bytes] uint8"""
    feat = np.ascontiguousarray(np.asarray(feat), dtype=np.float32)
    n, h, w, c = feat.shape
    payload, scales, total = _layout(fmt, h, w, c)
    wire = np.zeros((n, total), np.uint8)
    if fmt == "f32":
        wire[:] = feat.reshape(n, -1).view(np.uint8)
    elif fmt == "f16":
        with np.errstate(over="ignore"):                    # past 65520: +-Inf, as the contract says
            wire[:] = feat.reshape(n, -1).astype(np.float16).view(np.uint8)
    else:
        bits = feat.reshape(-1, BLOCK).view(np.uint32)
        e, bad = _block_scale(bits, _ELEM[fmt][3])
        code = np.where(bad[:, None], 0, _elem_codes(bits, e, fmt)).astype(np.uint8)
        if fmt == "mxfp4":
            code = code[:, 0::2] | (code[:, 1::2] << 4)
        wire[:, :payload] = code.reshape(n, payload)
        wire[:, payload:payload + scales] = np.where(bad, 0xFF, e + 127).astype(np.uint8).reshape(n, scales)
    return wire


def host_decode(wire, fmt, h, w, c):
    """wire [n, message_bytes] uint8 -> feat [n, h, w, c] float32"""
    wire = np.ascontiguousarray(np.asarray(wire), dtype=np.uint8)
    payload, scales, total = _layout(fmt, h, w, c)
    if wire.ndim != 2 or wire.shape[1] != total:
        raise ValueError("exchange: wire must be [n, %d] bytes for a %d x %d x %d %s map (got %s)"
                         % (total, h, w, c, fmt, tuple(wire.shape)))
    n = wire.shape[0]
    if fmt == "f32":
        return wire.view(np.float32).reshape(n, h, w, c).copy()
    if fmt == "f16":
        return wire.view(np.float16).astype(np.float32).reshape(n, h, w, c)
    code = wire[:, :payload]
    if fmt == "mxfp4":
        code = np.stack([code & 0xF, code >> 4], axis=-1)
    code = code.reshape(-1, BLOCK)
    scale = wire[:, payload:payload + scales].reshape(-1).astype(np.int64)
    v = _elem_values(code, scale - 127, fmt)
    v = np.where((scale == 0xFF)[:, None], np.float32(np.nan), v)
    return v.astype(np.float32).reshape(n, h, w, c)


CELLS_MAX = 16384                                           # DN_EXCHANGE_CELLS_MAX: one image's scores fit in 64 KiB of LDS
_BITS = {"f32": 32, "f16": 16, "mxfp8": 8, "mxfp4": 4}


def _check_cells(h, w, cells):
    P = h * w
    if min(h, w) <= 0 or P > CELLS_MAX:
        raise ValueError("exchange: a %d x %d map has %d cells, the selective exchange takes 1 .. %d" % (h, w, P, CELLS_MAX))
    if not 1 <= cells <= P:
        raise ValueError("exchange: cells = %d must be in [1, %d], the cells of a %d x %d map" % (cells, P, h, w))
    return P


def cells_message_bytes(fmt, h, w, c, cells):
    """bytes one agent sends per frame with capacity `cells` (dn_exchange_cells_message_bytes): the fixed-capacity message"""
    _check_cells(h, w, cells)
    return 16 + (2 * cells + 15) // 16 * 16 + _layout(fmt, 1, cells, c)[2]


def sent_bytes(fmt, c, count):
    """what a variable-length link would carry for `count` cells (a number, a mean included): the header, two bytes of
    index and the element bytes per cell, and for the MX formats one scale byte per 32 channels"""
    check_format(fmt)
    per_cell = 2 + c * _BITS[fmt] // 8 + (c // BLOCK if fmt in _ELEM else 0)
    return 16 + count * per_cell


def host_scores(feat):
    """feat [n, h, w, c] float32 -> score [n, h * w] uint32: the largest magnitude of a cell as its bit pattern"""
    feat = np.ascontiguousarray(np.asarray(feat), dtype=np.float32)
    n, h, w, c = feat.shape
    return (feat.reshape(n, h * w, c).view(np.uint32) & np.uint32(0x7fffffff)).max(axis=2)


def host_select(feat, cells):
    """feat [n, h, w, c] float32 -> (index [n, cells] uint16, count [n] int32): per image the first min(cells, non-zero
    cells) cells by (score descending, index ascending), listed in ascending index; 0xFFFF beyond count"""
    score = host_scores(feat).astype(np.int64)
    n, P = score.shape
    _check_cells(feat.shape[1], feat.shape[2], cells)
    index = np.full((n, cells), 0xFFFF, np.uint16)
    count = np.zeros(n, np.int32)
    for i in range(n):
        order = np.lexsort((np.arange(P), -score[i]))      # the last key is the primary one
        count[i] = min(cells, int((score[i] > 0).sum()))
        index[i, :count[i]] = np.sort(order[:count[i]])
    return index, count


def host_encode_cells(feat, fmt, cells):
    """feat [n, h, w, c] float32 -> wire [n, cells_message_bytes] uint8"""
    feat = np.ascontiguousarray(np.asarray(feat), dtype=np.float32)
    n, h, w, c = feat.shape
    total = cells_message_bytes(fmt, h, w, c, cells)
    index, count = host_select(feat, cells)
    body_at = 16 + (2 * cells + 15) // 16 * 16
    wire = np.zeros((n, total), np.uint8)
    wire[:, :4] = count.astype("<u4").view(np.uint8).reshape(n, 4)
    wire[:, 16:16 + 2 * cells] = index.astype("<u2").view(np.uint8).reshape(n, 2 * cells)
    rows = np.zeros((n, 1, cells, c), np.float32)
    cell = feat.reshape(n, h * w, c)
    for i in range(n):
        rows[i, 0, :count[i]] = cell[i, index[i, :count[i]]]
    wire[:, body_at:] = host_encode(rows, fmt)
    return wire


def host_decode_cells(wire, fmt, h, w, c, cells):
    """wire [n, cells_message_bytes] uint8 -> feat [n, h, w, c] float32: cell index[r] gets the dense decode of row r for
    r < min(count, cells), an index >= h * w is skipped, every other cell is +0.0"""
    wire = np.ascontiguousarray(np.asarray(wire), dtype=np.uint8)
    total = cells_message_bytes(fmt, h, w, c, cells)
    if wire.ndim != 2 or wire.shape[1] != total:
        raise ValueError("exchange: wire must be [n, %d] bytes for %d cells of a %d x %d x %d %s map (got %s)"
                         % (total, cells, h, w, c, fmt, tuple(wire.shape)))
    n, P = wire.shape[0], h * w
    body_at = 16 + (2 * cells + 15) // 16 * 16
    count = np.minimum(wire[:, :4].copy().view("<u4").reshape(n).astype(np.int64), cells)
    index = wire[:, 16:16 + 2 * cells].copy().view("<u2").reshape(n, cells).astype(np.int64)
    rows = host_decode(wire[:, body_at:], fmt, 1, cells, c).reshape(n, cells, c)
    feat = np.zeros((n, P, c), np.float32)
    for i in range(n):
        r = np.arange(count[i])
        r = r[index[i, :count[i]] < P]
        feat[i, index[i, r]] = rows[i, r]
    return feat.reshape(n, h, w, c)


def roundtrip(feat, fmt, cells=0, sent=None):
    """what a receiver decodes of `feat` [n, h, w, c] fp32 NHWC on the GPU.
    cells = 0: the whole map -- ops.exchange_encode + ops.exchange_decode, two launches; "f32" sends the map as it is:
    `feat` itself comes back and nothing is launched.
    cells = K > 0: the K strongest cells of every image, in any of the four formats -- ops.exchange_encode_cells +
    ops.exchange_decode_cells, four launches; `sent` (int64 [>= n] on the device, or None) takes each image's count."""
    check_format(fmt)
    if cells:
        n, h, w, c = feat.shape
        wire = ops.exchange_encode_cells(feat, fmt, cells, sent=sent)
        return ops.exchange_decode_cells(wire, fmt, h, w, c, cells)
    if fmt == "f32":
        return feat
    n, h, w, c = feat.shape
    return ops.exchange_decode(ops.exchange_encode(feat, fmt), fmt, h, w, c)
