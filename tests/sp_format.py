"""A host statement of the split-planar ("SP") f16 format in numpy: WHERE every 16-byte piece of an activation tensor and
of a plain packed weight image lies, and WHICH two binary16 bit patterns a float32 value becomes.  Written from the
format's description (include/disconet_hip.h "SP tensor", tests/conv_fp64.sp_split), not from the library's headers,
and it imports nothing from the library: tests/test_gpu_sp_format.py compares the bytes the kernels write with it.

A value x is stored as hi = half(clamp(x)), lo = half(clamp(x) - hi), clamp to +-65504 (x - hi is exact in float32).
A piece is 16 bytes = 8 binary16 = 8 consecutive channels: channels 16 * chunk + 8 * oct + 0..7.  The four pieces
("quarters") of a chunk are hi-oct0, hi-oct1, lo-oct0, lo-oct1: quarter = 2 * part + oct."""
import numpy as np

F16_MAX = np.float32(65504.0)


def split_bits(x):
    """float32 array -> (hi, lo) uint16 arrays: the bit patterns of tests/conv_fp64.sp_split's pair.  numpy rounds a
    float32 to binary16 to nearest-even, subnormals included, as the conversion instruction does."""
    v = np.clip(np.asarray(x, dtype=np.float32), -F16_MAX, F16_MAX)
    hi = v.astype(np.float16)
    lo = (v - hi.astype(np.float32)).astype(np.float16)
    return hi.view(np.uint16), lo.view(np.uint16)


def value_of(hi_bits, lo_bits):
    """float(hi) + float(lo) in float32: exact, what dn_sp_to_nhwc returns"""
    return hi_bits.view(np.float16).astype(np.float32) + lo_bits.view(np.float16).astype(np.float32)


def chunks_of(c):
    return (c + 15) // 16


# ---- the three index maps (piece = 16 bytes) ----------------------------------------------------
def act_piece(img, chunks, chunk, part, oct, hw, px):
    """SP activation tensor [image][chunk][4 quarters][hw]"""
    return ((img * chunks + chunk) * 4 + (2 * part + oct)) * hw + px


def weight_piece(block, part, oct, cout_pad, n):
    """SP packed weights [block][4 quarters][cout_pad]; a plain image has block = chunk * taps + tap"""
    return (block * 4 + (2 * part + oct)) * cout_pad + n


def frag_piece(nt, ks, ksteps, part, h, row):
    """A-operand fragment image [nt][ks][part][h][32 rows]"""
    return (((nt * ksteps + ks) * 2 + part) * 2 + h) * 32 + row


# ---- whole images -------------------------------------------------------------------------------
class _Image:
    """[pieces, 8] uint16 in which every piece is placed exactly once"""

    def __init__(self, pieces):
        self.bits = np.zeros((pieces, 8), np.uint16)
        self.placed = np.zeros(pieces, bool)

    def place(self, piece_index, bits):
        assert not self.placed[piece_index].any(), "a piece was placed twice"
        self.placed[piece_index] = True
        self.bits[piece_index] = bits

    def done(self):
        assert self.placed.all(), "a piece was never placed"
        return self.bits


def act_image(x):
    """x [n, h, w, c] float32 -> uint16 [pieces, 8]: the bytes of SpTensor.from_nhwc(x).data (padded channels are zero)"""
    n, h, w, c = x.shape
    chunks, hw = chunks_of(c), h * w
    full = np.zeros((n, hw, chunks * 16), np.float32)
    full[:, :, :c] = np.asarray(x, np.float32).reshape(n, hw, c)
    parts = split_bits(full)
    image = _Image(n * chunks * 4 * hw)
    px = np.arange(hw)
    for img in range(n):
        for chunk in range(chunks):
            for part in range(2):
                for oct in range(2):
                    c_first = 16 * chunk + 8 * oct
                    image.place(act_piece(img, chunks, chunk, part, oct, hw, px), parts[part][img, :, c_first:c_first + 8])
    return image.done()


def plain_weight_image(w, wmul, c0=None):
    """w [c_out, c_in, k, k] float32, wmul a power of two -> uint16 [pieces, 8]: dn_spconv_pack_weights' plain image.
    cout_pad = c_out rounded up to 64.  Chunks: those of source 0 (the first c0 input channels), then those of source 1,
    then zero chunks up to a multiple of four; outputs past c_out and input channels past a source's end are zero."""
    w = np.asarray(w, np.float32)
    c_out, c_in, k, _ = w.shape
    c0 = c_in if c0 is None else c0
    taps, cout_pad = k * k, (c_out + 63) // 64 * 64
    sources = [w[:, :c0], w[:, c0:]]
    chunks = (chunks_of(c0) + chunks_of(c_in - c0) + 3) // 4 * 4
    full = np.zeros((cout_pad, chunks * 16, taps), np.float32)
    first = 0
    for s in sources:
        full[:c_out, first:first + s.shape[1]] = s.reshape(c_out, s.shape[1], taps) * np.float32(wmul)
        first += chunks_of(s.shape[1]) * 16
    parts = split_bits(full)
    image = _Image(chunks * taps * 4 * cout_pad)
    n = np.arange(cout_pad)
    for chunk in range(chunks):
        for tap in range(taps):
            for part in range(2):
                for oct in range(2):
                    ci = 16 * chunk + 8 * oct
                    image.place(weight_piece(chunk * taps + tap, part, oct, cout_pad, n), parts[part][:, ci:ci + 8, tap])
    return image.done()


def nhwc_weight_image(w, split):
    """w [c_out, c_in, k, k] float32 -> the NHWC engine's image (dn_conv_pack_weights) as uint8 bytes:
    rows [chunk][tap][cout_pad] of kcp input channels, kcp = 16 (3x3) or 32 (1x1), cout_pad = c_out rounded up to 32.
    split False: a row is kcp float32; True: [kcp hi halves | kcp lo halves] in the same bytes."""
    w = np.asarray(w, np.float32)
    c_out, c_in, k, _ = w.shape
    taps, kcp, cout_pad = k * k, (16 if k == 3 else 32), (c_out + 31) // 32 * 32
    chunks = (c_in + kcp - 1) // kcp
    full = np.zeros((cout_pad, chunks * kcp, taps), np.float32)
    full[:c_out, :c_in] = w.reshape(c_out, c_in, taps)
    rows = full.reshape(cout_pad, chunks, kcp, taps).transpose(1, 3, 0, 2)      # [chunk][tap][co][k]
    if not split:
        return np.ascontiguousarray(rows).view(np.uint8).reshape(-1)
    hi, lo = split_bits(rows)
    return np.ascontiguousarray(np.concatenate([hi, lo], axis=-1)).view(np.uint8).reshape(-1)
