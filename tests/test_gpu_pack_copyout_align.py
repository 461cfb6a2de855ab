"""pack_cs_kernel's tile copy-out (pack.hip, copy_out_tile) at every output
alignment and capacity: 3-tile batches packed into an output tensor sliced
at each byte offset 0..15, with out_cap at the batch's end, 1, 15, 16 and 17
bytes short of it and inside the first tile.  Nothing at or past out_cap may
be written (canary bytes), and the bytes below it equal the oracle's prefix
(every tile here is staged, so the whole prefix is written)."""
import numpy as np
import pytest

import oracle_lib as O
import pack_check as P

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

NCH = 3 * P.TC
SEEDS = (0, 1, 3, 5, 6, 9, 10)  # (their 21 tile sizes take every residue mod 16)
CANARY = 0xA5


@pytest.fixture(scope="module")
def ctx():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from capnp_amd import Context
    c = Context(0)
    yield c
    c.close()


def _batch(seed):
    # random short tails: the tiles' byte counts take arbitrary residues mod 16
    rng = np.random.default_rng(100 + seed)
    sizes = rng.integers(100, 129, NCH)
    sizes[rng.integers(0, NCH)] = 0
    offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)
    return O.gen_fill(offs, kind0=seed % 3, pz=O.PZ30, id0=seed), offs


@pytest.fixture(scope="module")
def batches():
    out = {}
    for seed in SEEDS:
        words, offs = _batch(seed)
        ref = P.oracle(words, offs)
        assert P.unstaged_tiles(offs, ref[1]) == []
        out[seed] = (words, offs, ref)
    return out


def test_tile_sizes_cover_every_residue(batches):
    res = set()
    for _, _, (_, ref_offs, _) in batches.values():
        for t in range(3):
            res.add((int(ref_offs[(t + 1) * P.TC]) - int(ref_offs[t * P.TC])) % 16)
    assert res == set(range(16))


@pytest.mark.parametrize("seed", SEEDS)
def test_copyout_alignment_and_cap(ctx, batches, seed):
    words, offs, (ref, ref_offs, _) = batches[seed]
    total = len(ref)
    tile0 = int(ref_offs[P.TC])
    caps = [total, total - 1, total - 15, total - 16, total - 17, tile0 // 2 + 3]
    dw, do = P.dev(words), P.dev(offs)
    oo = torch.empty(NCH + 1, dtype=torch.int64, device="cuda")
    base = torch.empty(total + 64, dtype=torch.uint8, device="cuda")
    assert base.data_ptr() % 16 == 0
    for off in range(16):
        for cap in caps:
            base.fill_(CANARY)
            ctx.pack_batch_into(dw, do, base[off:off + cap], oo, chunks_per_tile=P.TC)
            got = base.cpu().numpy()
            assert np.array_equal(oo.cpu().numpy().view(np.uint64), ref_offs), (off, cap)
            assert (got[:off] == CANARY).all(), (off, cap)
            assert (got[off + cap:] == CANARY).all(), (off, cap)
            assert np.array_equal(got[off:off + cap], ref[:cap]), (off, cap)
