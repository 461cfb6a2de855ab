"""pack_cs_kernel<true>: the record sync index at every lane position.
Batches of 130 tiles of 16 chunks, so the look-back crosses a group edge at
tile 63; packed bytes, offsets and the whole index (every entry, the
unprovided ones of unstaged tiles included) must equal the oracle's."""
import numpy as np
import pytest

import oracle_lib as O
import pack_check as P

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

NCH = 130 * P.TC - 5  # 130 tiles, the last one short


@pytest.fixture(scope="module")
def ctx():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from capnp_amd import Context
    c = Context(0)
    yield c
    c.close()


def _offs(sizes):
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)


def _dense(rng, n):
    """Words without a zero byte (tag 0xFF: literal runs)."""
    return rng.integers(1, 2**63, n, dtype=np.uint64) | np.uint64(0x0101010101010101)


def _cycle():
    # lengths 1..128 cycling: a chunk starts at every word residue mod 8 and
    # the sync words fall on every lane
    sizes = np.arange(NCH) % 128 + 1
    offs = _offs(sizes)
    return O.gen_fill(offs, kind0=1, pz=O.PZ30), offs


def _runs():
    # zero runs and 0xFF runs of 9..127 words that start in words 0..63 and
    # reach into words 64..127, between single words of mixed tags; empty
    # chunks; a sync word that is itself a head falls out of the mixed words
    rng = np.random.default_rng(5)
    sizes = np.full(NCH, 128)
    sizes[rng.random(NCH) < 0.05] = 0
    short = np.nonzero(rng.random(NCH) < 0.1)[0]
    sizes[short] = rng.integers(1, 128, len(short))
    offs = _offs(sizes)
    words = O.gen_fill(offs, kind0=0, pz=O.PZ30)
    for c in range(NCH):
        a, n = int(offs[c]), int(sizes[c])
        if n < 128 or c % 4 == 3:
            continue
        lead = int(rng.integers(0, 64))
        run = int(rng.integers(9, 128))
        k = min(lead + run, n)
        if c % 4 == 0:
            words[a + lead:a + k] = 0
        elif c % 4 == 1:
            words[a + lead:a + k] = _dense(rng, k - lead)
        else:
            words[a + lead:a + k] = 0xFFFFFFFFFFFFFFFF
    return words, offs


def _unstaged():
    # as _cycle with one tile that holds a 129-word chunk and one tile of
    # 8.5-byte words that overflows its stage: no entries for either
    sizes = np.arange(NCH) % 128 + 1
    sizes[40 * P.TC + 3] = 129
    sizes[70 * P.TC:71 * P.TC] = 128
    sizes[5] = 0
    offs = _offs(sizes)
    words = O.gen_fill(offs, kind0=2, pz=O.PZ30)
    a, b = int(offs[70 * P.TC]), int(offs[71 * P.TC])
    words[a:b:2] = 0x1112131415161718
    words[a + 1:b:2] = 0x0000212223242526
    return words, offs


@pytest.mark.parametrize("make", [_cycle, _runs, _unstaged])
def test_sync_lanes(ctx, make):
    words, offs = make()
    ref = P.oracle(words, offs)
    if make is _unstaged:
        assert P.unstaged_tiles(offs, ref[1]) == [40, 70]
    else:
        assert P.unstaged_tiles(offs, ref[1]) == []
    P.check_pack(ctx, words, offs, True, ref=ref, exact_index=True)
    P.check_pack(ctx, words, offs, False, ref=ref)
