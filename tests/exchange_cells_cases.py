"""Shared inputs of the selective-exchange tests (tests/test_exchange_cells_host_cpu.py, tests/test_gpu_exchange_cells.py):
[n, h, w, c] float32 maps from seeded generators, built around what the selection of include/disconet_hip.h ("Selective
exchange") can get wrong -- empty cells, ties at the K boundary, fewer non-zero cells than K, -0.0, NaN / Inf -- and the
edge blocks of tests/exchange_cases.py laid out as cells.  Everything is numpy; nothing here touches the GPU."""
import numpy as np

from tests import exchange_cases as ec

F32 = np.float32


def relu_map(n, h, w, c, seed, empty=0.7):
    """a post-ReLU random map: about `empty` of the cells all zero, the others half zeros, half positive values with a
    binade of the cell's own (so that the cells' scores spread)"""
    rng = np.random.RandomState(seed)
    x = np.maximum(rng.randn(n, h, w, c), 0).astype(F32) * np.exp2(rng.randint(-6, 7, size=(n, h, w, 1))).astype(F32)
    x[rng.rand(n, h, w) < empty] = 0
    return x


def equal_scores(n, h, w, c, seed):
    """every cell's score is that of 1.0: one channel of its own is exactly 1.0, the others lie below 0.5"""
    rng = np.random.RandomState(seed)
    x = (rng.rand(n, h * w, c) * 0.5).astype(F32)
    x[np.arange(n)[:, None], np.arange(h * w)[None, :], rng.randint(0, c, size=(n, h * w))] = 1.0
    return x.reshape(n, h, w, c)


def tie_run(n, h, w, c, cells, seed):
    """a run of equal scores that straddles the K boundary: cells // 2 cells at scattered places score above 2.0 (all
    different), as many of the remaining cells as it takes to pass K -- again scattered -- score exactly 2.0, and the rest
    score below 1.0.  The cells taken from the run must be its lowest indices."""
    rng = np.random.RandomState(seed)
    P = h * w
    x = (rng.rand(n, P, c) * 0.9).astype(F32)
    above = cells // 2
    run = min(P - above, cells - above + max(1, min(cells, 7)))
    for i in range(n):
        order = rng.permutation(P)
        for j, p in enumerate(order[:above]):
            x[i, p, rng.randint(c)] = F32(3.0 + j)
        for p in order[above:above + run]:
            x[i, p, rng.randint(c)] = F32(-2.0 if rng.rand() < 0.5 else 2.0)      # the score is the magnitude
    return x.reshape(n, h, w, c)


def short_count(n, h, w, c, cells, seed):
    """with more than one image the last one is all zero; every other image has fewer than K non-zero cells (K // 2, none for
    K = 1), and among its empty cells one of only -0.0 and one of -0.0 and +0.0 mixed: neither is ever sent"""
    rng = np.random.RandomState(seed)
    P = h * w
    x = np.zeros((n, P, c), F32)
    for i in range(n if n == 1 else n - 1):
        order = rng.permutation(P)
        live = order[:cells // 2]
        x[i, live] = np.maximum(rng.randn(len(live), c), 0.01).astype(F32)
        rest = order[cells // 2:]
        if len(rest) > 0:
            x[i, rest[0]] = F32(-0.0)
        if len(rest) > 1:
            x[i, rest[1], ::2] = F32(-0.0)
    return x.reshape(n, h, w, c)


def negative_zero_only(n, h, w, c):
    """every value -0.0: nothing is sent, and the receiver sees +0.0"""
    return np.full((n, h, w, c), -0.0, F32)


def non_finite(n, h, w, c, seed):
    """relu_map with, per image, one cell that holds one NaN and one that holds one +-Inf (all their other values tiny), and
    one cell of only -0.0: the first two are selected before every finite cell"""
    rng = np.random.RandomState(seed)
    P = h * w
    x = relu_map(n, h, w, c, seed, empty=0.5).reshape(n, P, c)
    for i in range(n):
        order = rng.permutation(P)
        x[i, order[0]] = F32(1e-3)
        x[i, order[0], rng.randint(c)] = F32(np.nan)
        if P > 1:
            x[i, order[1]] = F32(1e-3)
            x[i, order[1], rng.randint(c)] = F32(np.inf if i % 2 == 0 else -np.inf)
        if P > 2:
            x[i, order[2]] = F32(-0.0)
    return x.reshape(n, h, w, c)


def edge_cells(n, h, w, c):
    """exchange_cases.edge_array()'s blocks laid out as cells: cell p of image i takes c / 32 consecutive edge blocks
    (cyclically, each image starting one block later), so every block meets every element format inside a sent cell"""
    edges = ec.edge_array()
    per_cell = c // ec.BLOCK
    blocks = n * h * w * per_cell
    which = (np.arange(blocks).reshape(n, -1) + np.arange(n)[:, None]) % len(edges)
    return edges[which.reshape(-1)].reshape(n, h, w, c).copy()


def named_inputs(n, h, w, c, cells, seed=0):
    """name -> [n, h, w, c] float32, in a fixed order: every input of the module at one shape and capacity"""
    return {
        "relu": relu_map(n, h, w, c, seed + 1),
        "equal_scores": equal_scores(n, h, w, c, seed + 2),
        "tie_run": tie_run(n, h, w, c, cells, seed + 3),
        "short_count": short_count(n, h, w, c, cells, seed + 4),
        "negative_zero_only": negative_zero_only(n, h, w, c),
        "non_finite": non_finite(n, h, w, c, seed + 5),
        "edges": edge_cells(n, h, w, c),
    }


def mixed(n, h, w, c, cells, seed=0):
    """[n, h, w, c]: image i is image i of named_inputs' (i mod 7)-th input"""
    kinds = list(named_inputs(n, h, w, c, cells, seed).values())
    return np.stack([kinds[i % len(kinds)][i] for i in range(n)])


def malformed_wires(fmt):
    """(x, its wire, the two malformed wires, (h, w, c, cells)): messages no encoder writes, but that the contract defines --
    a count far above K, and a last index >= P (still ascending)"""
    from disconet_amd import exchange as ex
    n, h, w, c, cells = 2, 3, 5, 64, 7
    x = equal_scores(n, h, w, c, seed=6)
    wire = ex.host_encode_cells(x, fmt, cells)
    assert wire[:, :4].view("<u4").reshape(-1).tolist() == [cells, cells]
    over = wire.copy()
    over[:, :4] = np.array([cells + 1000, 0xFFFFFFFF], "<u4").view(np.uint8).reshape(2, 4)
    past = wire.copy()
    past[:, 16 + 2 * (cells - 1):16 + 2 * cells] = np.array([h * w, h * w + 300], "<u2").view(np.uint8).reshape(2, 2)
    return x, wire, over, past, (h, w, c, cells)
