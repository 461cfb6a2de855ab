"""The rule of the record sync index (pack.hip, "Record sync index") in plain
Python against the oracle's index.

For the sync word m = 8 k of the batch, in chunk c at word i = m - offs[c]:
the covering record's head h is the last head at or below i, and the entry is
(pos[h] - chunk start) | (i - h) << 24.  The heads H and their positions are
read off the oracle's own packed bytes, so nothing here comes from the code
under test; `O.sync_index` is compared for every entry.
"""
import numpy as np
import pytest

import oracle_lib as O

SYNC = 8


def records(packed):
    """[(head word, pos, words, kind)] of one chunk's packed bytes; kind 0 a
    zero run, 1 a literal run (0xFF head), 2 a single word."""
    out, p, w = [], 0, 0
    while p < len(packed):
        tag = int(packed[p])
        if tag == 0:
            n = int(packed[p + 1])
            out.append((w, p, 1 + n, 0))
            p, w = p + 2, w + 1 + n
        elif tag == 0xFF:
            n = int(packed[p + 9])
            out.append((w, p, 1 + n, 1))
            p, w = p + 10 + 8 * n, w + 1 + n
        else:
            out.append((w, p, 1, 2))
            p, w = p + 1 + bin(tag).count("1"), w + 1
    assert p == len(packed)
    return out


def chunk_tables(packed, n):
    """H (bool per word) and pos (of the heads; chunk-relative)."""
    H = np.zeros(n, bool)
    pos = np.zeros(n, np.int64)
    for h, p, _, _ in records(packed):
        H[h] = True
        pos[h] = p
    assert not n or H[0]
    return H, pos


def rule_entry(H, pos, i):
    h = i
    while not H[h]:
        h -= 1
    return int(pos[h]) | ((i - h) << 24)


def _batches():
    rng = np.random.default_rng(11)
    # random fill at 30 % and 80 % zero words, lengths 0..128
    for seed, pz in ((1, O.PZ30), (2, O.PZ80)):
        sizes = rng.integers(0, 129, 300)
        offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)
        yield O.gen_fill(offs, kind0=seed % 3, pz=pz), offs
    # adversarial: runs of zeros and of 0xFF words of 9..127 words, heads in
    # the lower half with sync words in the upper, a sync word that is a head
    sizes, parts = [], []
    for run in list(range(9, 128, 7)) + [127]:
        for fill in (0, 0xFFFFFFFFFFFFFFFF, 0x0102030405060708):
            for lead in (0, 1, 5, 8, 60):
                w = rng.integers(1, 2**63, 128, dtype=np.uint64) | np.uint64(0x0101010101010101)
                w[::3] &= np.uint64(0x00FFFFFFFFFF00FF)
                k = min(lead + run, 128)
                w[lead:k] = fill
                n = int(rng.integers(k, 129))
                parts.append(w[:n])
                sizes.append(n)
    offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)
    yield np.concatenate(parts), offs


@pytest.mark.parametrize("which", [0, 1, 2])
def test_sync_rule_matches_oracle(which):
    words, offs = list(_batches())[which]
    st, packed, poffs = O.pack_batch(words, offs)
    assert st == 0
    ref = O.sync_index(packed, poffs, offs)
    assert O.sync_words() == SYNC
    seen = 0
    for c in range(len(offs) - 1):
        a, b = int(offs[c]), int(offs[c + 1])
        n = b - a
        H, pos = chunk_tables(packed[int(poffs[c]):int(poffs[c + 1])], n)
        first = -a % SYNC  # the chunk's first sync word
        for i in range(first, n, SYNC):
            k = (a + i) // SYNC
            want = int(ref[k])
            assert rule_entry(H, pos, i) == want, (c, i)
            seen += 1
    assert seen == len(ref) == -(-int(offs[-1]) // SYNC)
