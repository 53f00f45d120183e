"""The packed one-vector kernel's column loop keeps a second chunk in flight per wave (symv_kernels.h: SymvPackedSrc's ping / pong records,
symv1_tile's loop unrolled by two): what only that loop shape can get wrong, through admm_hip_test_symv_packed against the fp32 kernel
through admm_hip_test_symv_one, with NaN above the diagonal and a poison pattern in every plane (the helpers of test_gpu_symv_packed.py).

  * 1, 2, 3, 6 and 8 chunks per wave (tile widths 32, 64, 96, 192, 256): the minimum, the odd remainder, the longest ping-pong;
  * ragged edges: the chunk requested ahead lies beyond column p - 1 or beyond the last row;
  * diagonal tiles, whose lanes stop requesting chunk by chunk: their partial rows compared on their own;
  * escapes in a chunk that is decoded while the next one is in flight, and in the last chunk of a wave;
  * more tiles than resident slots; a forced "leave", which must still write nothing.
Everything is compared byte for byte: the packing is exact and the arithmetic behind the decode is the fp32 kernel's."""
import functools

import numpy as np
import pytest

from test_gpu_symv_packed import CAP, _expected_escapes, _fp32, _inverse_like, _options, _packed, _poisoned, _same_bytes, _tiles

pytestmark = pytest.mark.gpu

WIDTHS = [32, 64, 96, 192, 256]          # 1, 2, 3, 6, 8 chunks of 8 columns per wave


def _sched(width):
    return "%d,%d,0" % (width, width)


@functools.lru_cache(maxsize=None)
def _plan(p, width):
    tiles = _tiles(p, _sched(width))
    tiles.setflags(write=False)
    assert tiles[:, 2].max() == width and 2 * (tiles[:, 2] == width).sum() > len(tiles)      # (a strip's last segment may be narrower)
    return tiles


def _rule(A, p, width):
    """Escapes of A under this schedule by the NumPy rule (the base is per tile, so the count depends on the tile list)."""
    per_tile = _expected_escapes(A, _plan(p, width))
    assert per_tile.max() <= CAP
    return int(per_tile.sum())


@pytest.mark.parametrize("width", WIDTHS)
def test_every_chunk_count_per_wave_gives_the_fp32_kernels_bytes(width):
    p = 2304
    A, v0, v1 = _inverse_like(p)
    _same_bytes(A, v0, v1, _sched(width), _rule(A, p, width))


@pytest.mark.parametrize("width", [96, 256])
def test_ragged_edges_where_the_chunk_requested_ahead_does_not_exist(width):
    p = 2563                                  # 3 columns into the last group of 32, 3 rows into the last strip
    A, v0, v1 = _inverse_like(p)
    tiles = _plan(p, width)
    assert (tiles[:, 1] + tiles[:, 2] > p).any() and (tiles[:, 0] * 256 + 256 > p).any()
    _same_bytes(A, v0, v1, _sched(width), _rule(A, p, width))


@pytest.mark.parametrize("width", [64, 192, 256])
def test_diagonal_tiles_partial_rows(width):
    """In a tile on the diagonal a lane stops requesting at the chunk that lies wholly above its rows -- the chunk requested ahead
    as well -- and gets zeros: the dot row segment and the axpy row of every such tile, taken out of the planes, are the fp32 kernel's and
    hold no NaN of the upper triangle."""
    p = 2304
    A, v0, v1 = _inverse_like(p)
    tiles = _plan(p, width)
    nrb = -(-p // 256)
    diagonal = tiles[tiles[:, 1] + tiles[:, 2] > tiles[:, 0] * 256]
    assert len(diagonal) >= nrb
    with _options(_sched(width)):
        _, dot, axp, ntiles, left = _fp32(A, v0, v1, 0)
        _, dotp, axpp, ntilesp, leftp, (_, over, _, ran) = _packed(A, v0, v1, 0)
    assert (ntiles, left, leftp, over, ran) == (ntilesp, 0, 0, 0, 1)
    ldo = dot.shape[1] // nrb
    assert ldo * nrb == dot.shape[1] and axp.shape[1] % ldo == 0
    d, dp = dot[0].reshape(nrb, ldo), dotp[0].reshape(nrb, ldo)
    x, xp = axp[0].reshape(-1, ldo), axpp[0].reshape(-1, ldo)
    for rb, c0, w, seg in diagonal:
        a, b = dp[rb, c0:c0 + w], xp[seg, rb * 256:rb * 256 + 256]
        assert np.isfinite(a).all() and np.isfinite(b).all(), (rb, c0)
        assert a.tobytes() == d[rb, c0:c0 + w].tobytes(), (rb, c0)
        assert b.tobytes() == x[seg, rb * 256:rb * 256 + 256].tobytes(), (rb, c0)


def _plant_every_chunk(p, width):
    """The inverse-like matrix with one entry replaced in EVERY chunk of every wave of an interior tile and of a diagonal tile (below the
    diagonal): denormals and entries 2^-40 below their neighbours (escapes) in turn with exact zeros (a code of their own).  An escape
    then falls in each chunk that is decoded while the next is in flight, and in the last chunk of each wave."""
    A, v0, v1 = _inverse_like(p)
    A = A.copy(order="F")
    tiles = _plan(p, width)
    nrb = -(-p // 256)
    interior = tiles[(tiles[:, 1] + tiles[:, 2] <= tiles[:, 0] * 256) & (tiles[:, 0] == nrb - 2)][0]
    diagonal = tiles[(tiles[:, 1] + tiles[:, 2] > tiles[:, 0] * 256) & (tiles[:, 0] == nrb // 2)][-1]
    kinds = [np.uint32(0x00012345).view(np.float32), np.float32(3e-3 * 2.0 ** -40), np.float32(0.0), np.float32(-3e-3 * 2.0 ** -40)]
    planted = 0
    for rb, c0, w, _ in (interior, diagonal):
        cw = w // 4
        for wave in range(4):
            for q in range(cw // 8):
                c = c0 + wave * cw + q * 8 + (q + wave) % 8
                r = max(rb * 256 + 255 - ((5 * q + 3 * wave) % 16), c)    # the last 16 rows of the strip, or the diagonal entry of the column
                assert c <= r < min(rb * 256 + 256, p)
                val = kinds[(q + wave) % 4]
                A[r, c] = val
                planted += val != 0
    return A, v0, v1, tiles, int(planted)


@pytest.mark.parametrize("width", [64, 96, 192, 256])
def test_escapes_in_every_chunk_of_a_wave(width):
    p = 2304
    A, v0, v1, tiles, planted = _plant_every_chunk(p, width)
    per_tile = _expected_escapes(A, tiles)
    base = int(_expected_escapes(_inverse_like(p)[0], tiles).sum())
    assert int(per_tile.sum()) == base + planted and planted >= 2 * 3 * (width // 32) // 4 and per_tile.max() <= CAP
    _same_bytes(A, v0, v1, _sched(width), base + planted)


def test_more_tiles_than_resident_slots():
    p, width = 4200, 32                       # 1220 tiles: the later ones start on freed slots, beside tiles in every phase of their loop
    A, v0, v1 = _inverse_like(p)
    assert len(_plan(p, width)) == 1220
    _same_bytes(A, v0, v1, _sched(width), _rule(A, p, width))


@pytest.mark.parametrize("width", [96, 256])
def test_a_forced_leave_writes_no_partial_and_counts_every_tile(width):
    p = 2563
    A, v0, v1 = _inverse_like(p)
    with _options(_sched(width)):
        for nt in (0, 1):
            _, dot, axp, tiles, left, (met, over, _, ran) = _packed(A, v0, v1, 2, nt)
            assert _poisoned(dot) and _poisoned(axp)
            assert left == tiles == len(_plan(p, width)) and (over, ran) == (0, 1)
            assert met == _rule(A, p, width)
