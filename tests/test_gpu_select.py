"""GPU parity of the selective unpack (capnp_gpu_unpack_batch_select,
Context.unpack_select_into): entry i of a selection must be the batch decode
of chunk ids[i] of the store.

The expected result is the oracle's: the whole store is decoded once on the
CPU (oracle_lib.unpack_batch) and its words, statuses and consumed counts are
indexed by the ids; the expected offsets are the running sum of the selected
lengths.  Compared: the offsets in full, every status, and consumed and the
words of every entry whose oracle status is 0.
Reference: serialize_packed.rs:80-228 (PackedRead::read), io.rs:16-31
(read_exact)."""
import numpy as np
import pytest

import oracle_lib as O

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SENTINEL = 0x5A5A5A5A5A5A5A5A
EDGE_COUNTS = [0, 1, 2, 7, 8, 9, 63, 64, 65, 127, 128, 129, 255, 256, 257, 258, 511, 512, 513,
               1024, 2047, 2048, 2049, 4096, 8192, 0, 70000]
EDGE_SEED = 4100  # (the packed starts of this seed cover >= 8 residues mod 16: asserted below)


@pytest.fixture(scope="module")
def ctx():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from capnp_amd import Context
    c = Context(0)
    yield c
    c.close()


def _i64(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64).copy()).cuda()


class Store:
    """A packed store on the host and the device, and its oracle decode."""

    def __init__(self, packed, in_off, word_off, sync=None):
        self.packed = np.ascontiguousarray(packed, np.uint8)
        self.in_off = np.ascontiguousarray(in_off, np.uint64)
        self.word_off = np.ascontiguousarray(word_off, np.uint64)
        self.n = len(self.in_off) - 1
        self.words, self.status, self.consumed = O.unpack_batch(self.packed, self.in_off,
                                                                self.word_off)
        self.lens = np.diff(self.word_off.astype(np.int64))
        self.sync = sync
        if torch.cuda.is_available():
            self.d_packed = torch.from_numpy(self.packed.copy()).cuda()
            self.d_in_off = _i64(self.in_off)
            self.d_word_off = _i64(self.word_off)

    def expected(self, ids):
        """-> (offsets, status, consumed, words, per-word 'entry decodes' mask)
        for ids that all lie in the store."""
        ids = np.asarray(ids, np.int64)
        lens = self.lens[ids] if len(ids) else np.zeros(0, np.int64)
        off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        total = int(off[-1])
        # word k of the output = store word src0[e] + (k - off[e]) of its entry e
        e = np.repeat(np.arange(len(ids)), lens)
        src = self.word_off[ids].astype(np.int64)[e] + (np.arange(total) - off[e]) if total \
            else np.zeros(0, np.int64)
        st = self.status[ids] if len(ids) else np.zeros(0, np.int32)
        return (off, st, self.consumed[ids].astype(np.int64) if len(ids) else
                np.zeros(0, np.int64), self.words[src], (st == 0)[e] if total else
                np.zeros(0, bool))


def _sync_forms(store, seed=5):
    """None, the true index, all 0xFFFFFFFF, and 5 % of the entries XORed
    with random bits."""
    true = store.sync
    rng = np.random.default_rng(seed)
    dmg = true.copy()
    hit = rng.random(len(dmg)) < 0.05
    dmg[hit] ^= rng.integers(1, 1 << 32, int(hit.sum()), dtype=np.uint64).astype(np.uint32)
    return [("none", None), ("true", true), ("allff", np.full_like(true, 0xFFFFFFFF)),
            ("xor5", dmg)]


def _run(ctx, store, ids, sync=None, cap=None, slack=64):
    """One unpack_select_into over a sentinel-filled output of the needed
    size + slack (or cap + slack when cap is given: the call is told cap).
    -> (words incl. slack, offsets, status, consumed) as numpy arrays."""
    ids = np.asarray(ids, np.int64)
    nsel = len(ids)
    inside = ids[(ids >= 0) & (ids < store.n)]
    need = int(store.lens[inside].sum()) if len(inside) else 0
    told = need if cap is None else cap
    buf = torch.full((told + slack,), SENTINEL, dtype=torch.int64, device="cuda")
    off = torch.full((nsel + 1,), -1, dtype=torch.int64, device="cuda")
    st = torch.full((max(nsel, 1),), -7, dtype=torch.int32, device="cuda")
    cons = torch.full((max(nsel, 1),), -7, dtype=torch.int64, device="cuda")
    d_sync = None if sync is None else torch.from_numpy(sync.view(np.int32).copy()).cuda()
    ctx.unpack_select_into(store.d_packed, store.d_in_off, store.d_word_off,
                           torch.from_numpy(ids.copy()).cuda(), buf[:told], off, st, cons,
                           sync=d_sync)
    torch.cuda.synchronize()
    return (buf.cpu().numpy().view(np.uint64), off.cpu().numpy(), st.cpu().numpy()[:nsel],
            cons.cpu().numpy()[:nsel])


def _check(store, ids, got, what):
    words, off, st, cons = got
    eo, es, ec, ew, ok = store.expected(ids)
    assert np.array_equal(off, eo), (what, "offsets")
    assert np.array_equal(st, es), (what, "status", np.nonzero(st != es)[0][:8])
    good = es == 0
    assert np.array_equal(cons[good], ec[good]), (what, "consumed")
    total = int(eo[-1])
    bad = np.nonzero((words[:total] != ew) & ok)[0]
    assert len(bad) == 0, (what, "words", bad[:8])
    assert (words[total:] == SENTINEL).all(), (what, "wrote past the total")


# ---------------------------------------------------------------------------

@pytest.fixture(scope="module")
def edge():
    offs = np.concatenate([[0], np.cumsum(EDGE_COUNTS)]).astype(np.uint64)
    kinds = (np.arange(len(EDGE_COUNTS)) % 3).astype(np.uint8)
    words = O.gen_fill(offs, kinds=kinds, pz=O.PZ30, id0=EDGE_SEED)
    st, packed, poff = O.pack_batch(words, offs)
    assert st == 0
    # (before any GPU call) the chunks start at many misalignments
    assert len(set(int(p) % 16 for p in poff[:-1])) >= 8
    s = Store(packed, poff, offs, O.sync_index(packed, poff, offs))
    assert (s.status == 0).all() and np.array_equal(s.words, words)
    return s


def _edge_selections(n):
    rng = np.random.default_rng(77)
    return {
        "identity": np.arange(n),
        "reversed": np.arange(n)[::-1],
        "twice": np.repeat(np.arange(n), 2),
        "id11x300": np.full(300, 11),
        "empties": np.array([0, 25]),
        "single": np.array([20]),
        "none": np.zeros(0, np.int64),
        "random1000": rng.integers(0, n, 1000),
    }


@pytest.mark.parametrize("sel", ["identity", "reversed", "twice", "id11x300", "empties", "single",
                                 "none", "random1000"])
def test_edge_store(ctx, edge, sel):
    """Chunk sizes around every table limit (the 255-word run cap, the 64-word
    groups, the 2048-word tile, chunks past the tile and past the long-unit
    window), zero runs and literal runs, in every order; with no index, the
    true one and two damaged ones: all equal the oracle."""
    assert EDGE_COUNTS[11] == 129 and EDGE_COUNTS[0] == 0 and EDGE_COUNTS[25] == 0
    ids = _edge_selections(edge.n)[sel]
    for name, sync in _sync_forms(edge):
        _check(edge, ids, _run(ctx, edge, ids, sync=sync), (sel, name))


def _clean(nw, seed, kind=0):
    w = O.gen_fill(np.array([0, nw], np.uint64), kinds=np.array([kind], np.uint8), id0=seed)
    st, b = O.pack(w.view(np.uint8))
    assert st == 0
    return b


@pytest.fixture(scope="module")
def malformed():
    vec = [
        (bytes([0xf0, 1, 2]), 25), (bytes([0]), 25), (bytes([0xff] + list(range(1, 9))), 25),
        (bytes([1, 1]), 25), (bytes([0xff] + list(range(1, 9)) + [37, 1, 2]), 1),
        (_clean(200, 31)[:-3], 200),          # cut 3 bytes short
        (_clean(96, 32, kind=1), 96 + 8),     # claims 8 more words than it holds
        # (beyond the list above: a literal run without its bytes and an empty
        # chunk that claims words, FailedToFillTheWholeBuffer)
        (bytes([0xff] + list(range(1, 9)) + [2] + [7] * 11), 3), (b"", 5),
    ]
    chunks = []
    for k, v in enumerate(vec):
        nw = [33, 128, 5, 300, 64, 1, 129, 9, 2050][k]
        chunks.append((_clean(nw, 40 + k, kind=k % 3), nw))
        chunks.append(v)
    chunks.append((_clean(77, 60), 77))
    packed = np.frombuffer(b"".join(c[0] for c in chunks), np.uint8)
    in_off = np.concatenate([[0], np.cumsum([len(c[0]) for c in chunks])]).astype(np.uint64)
    word_off = np.concatenate([[0], np.cumsum([c[1] for c in chunks])]).astype(np.uint64)
    s = Store(packed, in_off, word_off)
    assert (s.status[0::2] == 0).all() and (s.status[1::2] != 0).all()
    assert set(s.status[1::2]) >= {2, 3, 4}
    return s


def test_malformed_store(ctx, malformed):
    """The reference's error vectors, a truncated chunk and an over-claiming
    chunk between clean chunks, selected in a mixed order with repeats: every
    status and consumed count is the oracle's, the clean neighbours' words are
    intact and nothing is written past the total.  Such a store has no true
    index; an absent, an empty and a garbage one must all give the oracle's
    results (the index is never trusted)."""
    n = malformed.n
    rng = np.random.default_rng(9)
    ids = np.concatenate([np.arange(n)[::-1], rng.integers(0, n, 60), np.arange(n),
                          [1, 1, 3, 3, 0, 13, 13, 17, 17]])
    ne = -(-int(malformed.word_off[-1]) // O.sync_words())
    # garbage entries with small offsets and run lengths, so that many pass
    # the range checks and are walked from
    small = (rng.integers(0, 600, ne) | (rng.integers(0, 4, ne) << 24)).astype(np.uint32)
    for name, sync in (("none", None), ("allff", np.full(ne, 0xFFFFFFFF, np.uint32)),
                       ("random", rng.integers(0, 1 << 32, ne, dtype=np.uint64).astype(np.uint32)),
                       ("small", small)):
        _check(malformed, ids, _run(ctx, malformed, ids, sync=sync), ("malformed", name))


def test_invalid_ids(ctx, edge):
    """Ids outside the store in the middle of a valid list: status 64, zero
    words, consumed 0; the other entries are unaffected."""
    n = edge.n
    valid = np.array([3, 12, 26, 0, 7, 19, 19, 5], np.int64)
    ids = np.concatenate([valid[:4], [n, n + 5, -2**63], valid[4:]]).astype(np.int64)
    words, off, st, cons = _run(ctx, edge, ids)
    bad = np.array([4, 5, 6])
    assert (st[bad] == 64).all() and (cons[bad] == 0).all()
    assert (off[bad + 1] == off[bad]).all()
    keep = np.setdiff1d(np.arange(len(ids)), bad)
    # without the invalid entries the result is the valid list's
    off_v = np.concatenate([off[keep], off[-1:]])
    _check(edge, ids[keep], (words, off_v, st[keep], cons[keep]), "invalid ids")


def test_invalid_store_offsets(ctx, edge):
    """A chunk whose byte or word offsets decrease fails alone (status 64,
    zero words), whatever its neighbours; the store is not scanned."""
    in_off = edge.in_off.copy()
    word_off = edge.word_off.copy()
    s = Store(edge.packed, in_off, word_off)
    bo = in_off.copy()
    bo[10] = bo[11] + 1      # chunk 10: bytes decrease (chunk 9 then over-reads: not selected)
    wo = word_off.copy()
    wo[15] = wo[16] + 3      # chunk 15: words decrease
    s.d_in_off, s.d_word_off = _i64(bo), _i64(wo)
    ids = np.array([2, 10, 12, 15, 20, 10], np.int64)
    words, off, st, cons = _run(ctx, s, ids)
    bad = np.array([1, 3, 5])
    assert (st[bad] == 64).all() and (cons[bad] == 0).all() and (off[bad + 1] == off[bad]).all()
    keep = np.array([0, 2, 4])
    off_v = np.concatenate([off[keep], off[-1:]])
    assert off[-1] == s.lens[[2, 12, 20]].sum()
    _check(s, ids[keep], (words, off_v, st[keep], cons[keep]), "decreasing offsets")


@pytest.mark.parametrize("k,into", [(5, 1), (9, 100), (3, 0), (12, 2048)])
def test_short_words_cap(ctx, edge, k, into):
    """words_cap ends `into` words inside entry k: the entries before are
    exact, entry k and every later entry whose range ends past the cap get
    status 9, nothing at or past the cap is written and the offsets are
    complete."""
    ids = np.array([12, 3, 21, 9, 0, 17, 25, 11, 2, 22, 14, 1, 26, 6, 25, 4], np.int64)
    eo, es, ec, ew, _ = edge.expected(ids)
    assert eo[k] + into < eo[k + 1]
    cap = int(eo[k]) + into
    words, off, st, cons = _run(ctx, edge, ids, cap=cap)
    assert np.array_equal(off, eo)
    short = eo[1:] > cap
    assert short[k] and not short[:k].any()
    assert np.array_equal(st[~short], es[~short]) and (st[short] == 9).all()
    assert np.array_equal(cons[~short], ec[~short])
    assert np.array_equal(words[:int(eo[k])], ew[:int(eo[k])])
    assert (words[cap:] == SENTINEL).all()


@pytest.fixture(scope="module")
def tiles():
    n, nw = 4096, 128
    offs = (np.arange(n + 1) * nw).astype(np.uint64)
    words = O.gen_fill(offs, kind0=0, pz=O.PZ30, id0=900)
    st, packed, poff = O.pack_batch(words, offs)
    assert st == 0
    return Store(packed, poff, offs, O.sync_index(packed, poff, offs))


@pytest.mark.parametrize("sel", ["permutation", "replace16384"])
def test_many_tiles(ctx, tiles, sel):
    """A 4,096 x 128-word config-2 store with its index: a random
    permutation of all ids, and 16,384 ids with replacement."""
    rng = np.random.default_rng(2024)
    ids = rng.permutation(tiles.n) if sel == "permutation" else rng.integers(0, tiles.n, 16384)
    for name, sync in (("none", None), ("true", tiles.sync)):
        _check(tiles, ids, _run(ctx, tiles, ids, sync=sync), (sel, name))


def test_unpack_select_sizes_its_output(ctx, edge):
    """Context.unpack_select: the output is sized from the offsets."""
    ids = np.array([26, 4, 4, 18, 25, 13], np.int64)
    d_sync = torch.from_numpy(edge.sync.view(np.int32).copy()).cuda()
    w, off, st, cons = ctx.unpack_select(edge.d_packed, edge.d_in_off, edge.d_word_off,
                                         torch.from_numpy(ids).cuda(), sync=d_sync)
    torch.cuda.synchronize()
    eo = edge.expected(ids)[0]
    assert w.numel() == eo[-1] and off.numel() == len(ids) + 1
    got = (np.concatenate([w.cpu().numpy().view(np.uint64), [np.uint64(SENTINEL)]]),
           off.cpu().numpy(), st.cpu().numpy(), cons.cpu().numpy())
    _check(edge, ids, got, "unpack_select")


def test_stream_order(ctx, tiles):
    """Two calls back to back on a non-default stream and a torch op on that
    stream that consumes the words, with no host synchronisation in between:
    the results are the oracle's."""
    rng = np.random.default_rng(31)
    sel = [rng.integers(0, tiles.n, 3000), rng.permutation(tiles.n)[:2500]]
    ctx.reserve(4096)  # (the workspace covers both selections: no growth, no wait)
    exp = [tiles.expected(ids) for ids in sel]
    d_ids = [torch.from_numpy(ids).cuda() for ids in sel]
    d_sync = torch.from_numpy(tiles.sync.view(np.int32).copy()).cuda()
    bufs = [torch.full((int(e[0][-1]),), SENTINEL, dtype=torch.int64, device="cuda") for e in exp]
    offs = [torch.empty(len(ids) + 1, dtype=torch.int64, device="cuda") for ids in sel]
    sts = [torch.empty(len(ids), dtype=torch.int32, device="cuda") for ids in sel]
    cons = [torch.empty(len(ids), dtype=torch.int64, device="cuda") for ids in sel]
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        for j in range(2):
            ctx.unpack_select_into(tiles.d_packed, tiles.d_in_off, tiles.d_word_off, d_ids[j],
                                   bufs[j], offs[j], sts[j], cons[j], sync=d_sync)
        copies = [b.clone() for b in bufs]
        folded = [(b >> 1).sum() for b in bufs]
    s.synchronize()
    for j in range(2):
        eo, es, ec, ew, _ = exp[j]
        assert np.array_equal(offs[j].cpu().numpy(), eo)
        assert np.array_equal(sts[j].cpu().numpy(), es) and (es == 0).all()
        assert np.array_equal(cons[j].cpu().numpy(), ec)
        assert np.array_equal(copies[j].cpu().numpy().view(np.uint64), ew)
        assert int(folded[j].item()) == int((ew.view(np.int64) >> 1).sum())
