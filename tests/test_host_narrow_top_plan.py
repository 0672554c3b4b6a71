"""The slab-row map of the top layer's target pass inside the block forward launch (csrc/gadapt_block_plan.h: gadapt_block_slab_plan,
gadapt_block_owned_block - through their host copies), checked against the two layouts it joins:

 - the standalone launch it replaces gives slab row r the nodes 256 r .. 256 r + 255, summed as (b0 + b1) + (b2 + b3) over the row's
   four 64-node blocks in node order, and writes every one of the `gadapt_backward_slab_rows` rows;
 - the block kernel's wave w owns frame block w or w + 8 - the one that starts at or behind the owned range - of a frame that begins
   `margin` = K halo rounded up to 64 nodes ahead of the tile (restated below from the kernel's documentation, not from the plan).

For every N from 1 to a few thousand, sizes around the 512-row cap and the headline N, every halo and group size the plan accepts: each
row that has nodes is fed by exactly its four blocks in node order, every row of the slab is written by exactly one tile, and no row
index reaches the row count."""
import ctypes as C

import pytest

from g_adaptivity_amd import _native

TILE, BLOCK, ROW_NODES = 512, 64, 256
SIZES = list(range(1, 2200)) + [4095, 4096, 4097, 12450, 36864, 65535, 65537, 130561, 131071, 131072]


def _plan(n, halo, layers, tile):
    out = (C.c_int32 * 12)()
    assert _native.lib().gadapt_narrow_block_slab_plan_host(n, halo, layers, tile, C.addressof(out)) == 0
    v = list(out)
    return v[0:2], [v[2:6], v[6:10]], v[10], v[11]


def _owned_start(halo, layers, tile, wave):
    """First node of the 64-node block wave `wave` of tile `tile` owns, from the frame's rule."""
    margin = -(-layers * halo // 64) * 64
    so = 1 if 64 * wave < margin else 0
    return TILE * tile - margin + BLOCK * wave + TILE * so


@pytest.mark.parametrize("halo", [32, 64])
@pytest.mark.parametrize("layers", [1, 2, 3, 4])
def test_owned_blocks_are_the_tile_in_rotated_order(halo, layers):
    lib = _native.lib()
    blocks = [lib.gadapt_narrow_block_owned_block_host(halo, layers, w) for w in range(8)]
    assert sorted(blocks) == list(range(8))
    for tile in (0, 1, 255):
        for w in range(8):
            assert _owned_start(halo, layers, tile, w) == TILE * tile + BLOCK * blocks[w], (tile, w)


@pytest.mark.parametrize("halo", [32, 64])
@pytest.mark.parametrize("layers", [1, 2, 3, 4])
def test_every_slab_row_is_written_once_and_fed_by_its_four_blocks(halo, layers):
    lib = _native.lib()
    for n in SIZES:
        rows = lib.gadapt_backward_slab_rows(n, 64)
        assert n <= ROW_NODES * rows                                     # the eligibility rule: one node per lane of the standalone launch
        n_tiles, busy = -(-n // TILE), -(-n // ROW_NODES)
        written = [0] * rows
        for tile in range(n_tiles):
            own, waves, zero_first, zero_step = _plan(n, halo, layers, tile)
            assert own == [2 * tile, 2 * tile + 1]
            for j, r in enumerate(own):
                assert 0 <= r < rows, (n, tile, r, rows)
                written[r] += 1
                if r < busy:
                    starts = [_owned_start(halo, layers, tile, w) for w in waves[j]]
                    assert starts == [ROW_NODES * r + BLOCK * b for b in range(4)], (n, tile, r, starts)
                assert sorted(waves[j]) == sorted(set(waves[j])) and all(0 <= w < 8 for w in waves[j])
            assert zero_step >= 1 and zero_first >= 2 * n_tiles
            for r in range(zero_first, rows, zero_step):
                assert r >= busy                                         # only rows without nodes are zero-filled
                written[r] += 1
        assert written == [1] * rows, (n, [r for r, k in enumerate(written) if k != 1][:8])


def test_bad_arguments():
    lib = _native.lib()
    out = (C.c_int32 * 12)()
    for args in ((0, 32, 4, 0), (1000, 48, 4, 0), (1000, 32, 5, 0), (1000, 32, 0, 0), (1000, 32, 4, 2), (1000, 32, 4, -1)):
        assert lib.gadapt_narrow_block_slab_plan_host(*args, C.addressof(out)) == -1, args
    assert lib.gadapt_narrow_block_slab_plan_host(1000, 32, 4, 0, None) == -1
    for args in ((48, 4, 0), (32, 5, 0), (32, 4, 8), (32, 4, -1)):
        assert lib.gadapt_narrow_block_owned_block_host(*args) == -1, args
