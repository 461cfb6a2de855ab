"""One context packing batch after batch: the look-back records and overflow
flags in its workspace are left zero by each chunk-tile pack for the next
(pack.hip, pack_ovf_kernel), and zeroed by the call wherever that is not
known (the gap pack and the word tiles use the same workspace).  A stale
record or flag would shift offsets or drop a tile's bytes: every result is
compared with the oracle."""
import numpy as np
import pytest

import oracle_lib as O
import pack_check as P

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


def _ctx():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from capnp_amd import Context
    return Context(0)


def _offs(sizes):
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)


def _plain(seed, nchunks, lo=60, hi=129):
    rng = np.random.default_rng(seed)
    offs = _offs(rng.integers(lo, hi, nchunks))
    return O.gen_fill(offs, kind0=seed % 3, pz=O.PZ30), offs


def _overflowing(seed, nchunks):
    # tiles with a chunk over 128 words and tiles of 8.5-byte words: both set
    # their overflow flag and leave their bytes to pack_ovf_kernel
    rng = np.random.default_rng(seed)
    sizes = rng.integers(60, 129, nchunks)
    sizes[::37] = rng.integers(129, 400, len(sizes[::37]))
    offs = _offs(sizes)
    words = O.gen_fill(offs, kind0=1, pz=O.PZ30)
    for t in range(2, nchunks // P.TC, 9):
        sizes_t = slice(int(offs[t * P.TC]), int(offs[(t + 1) * P.TC]))
        w = words[sizes_t]
        w[0::2] = 0x1112131415161718
        w[1::2] = 0x0000212223242526
    return words, offs


def _check_messages(ctx, seed, nmsg):
    rng = np.random.default_rng(seed)
    msgs = []
    for i in range(nmsg):
        lens = [128] if i % 7 else [60, 68]
        msgs.append([O.gen_fill(_offs([n]), kind0=0, pz=O.PZ30, id0=int(rng.integers(1 << 30)))
                     for n in lens])
    seg_off = _offs([len(s) for m in msgs for s in m]).astype(np.int64)
    msg_seg_off = _offs([len(m) for m in msgs]).astype(np.int64)
    words = np.concatenate([s for m in msgs for s in m])
    packed, mo = ctx.write_messages(P.dev(words), torch.from_numpy(seg_off).cuda(),
                                    torch.from_numpy(msg_seg_off).cuda())
    torch.cuda.synchronize()
    ref = b"".join(O.write_message(m)[1] for m in msgs)
    assert packed.cpu().numpy().tobytes() == ref
    assert int(mo[-1].item()) == len(ref)


@pytest.mark.parametrize("sync", [False, True])
def test_state_reuse_sequence(sync):
    ctx = _ctx()
    try:
        big = _plain(1, 400 * P.TC + 3)
        ref_big = P.check_pack(ctx, *big, sync)
        P.check_pack(ctx, *big, sync, ref=ref_big)              # the state the first call left
        P.check_pack(ctx, *_plain(2, 50 * P.TC), sync)          # a smaller batch
        ovf = _overflowing(3, 120 * P.TC)
        ref_ovf = P.oracle(*ovf)
        assert len(P.unstaged_tiles(ovf[1], ref_ovf[1])) > 20
        P.check_pack(ctx, *ovf, sync, ref=ref_ovf)              # sets overflow flags
        P.check_pack(ctx, *_plain(4, 150 * P.TC), sync)         # ... which must be gone here
        _check_messages(ctx, 5, 600)                            # the gap pack
        P.check_pack(ctx, *big, sync, ref=ref_big)
        long_ = _plain(6, 40, 1500, 2500)                       # word tiles (mean >= 512 words)
        P.check_pack(ctx, *long_, sync, chunks_per_tile=0)
        P.check_pack(ctx, *big, sync, ref=ref_big)
        P.check_pack(ctx, *_plain(7, 3000, 20, 60), sync, chunks_per_tile=32)  # the lean kernel
        P.check_pack(ctx, *big, sync, ref=ref_big)
    finally:
        ctx.close()


def test_state_grows_between_calls():
    ctx = _ctx()
    try:
        P.check_pack(ctx, *_plain(8, 10 * P.TC), True)
        ctx.reserve(1 << 21)  # a larger workspace: allocated (and zeroed) anew
        P.check_pack(ctx, *_plain(9, 300 * P.TC + 1), True)
        P.check_pack(ctx, *_plain(8, 10 * P.TC), True)
    finally:
        ctx.close()


class _Captured:
    """A pack with the index captured into a graph, and its oracle."""

    def __init__(self, ctx, words, offs):
        self.ref = P.oracle(words, offs)
        n, total = len(offs) - 1, int(offs[-1])
        self.dw, self.do = P.dev(words), P.dev(offs)
        self.out = torch.empty(ctx.batch_bound_bytes(total, n), dtype=torch.uint8, device="cuda")
        self.oo = torch.empty(n + 1, dtype=torch.int64, device="cuda")
        self.sy = torch.empty(ctx.sync_entries(total), dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            ctx.pack_batch_into(self.dw, self.do, self.out, self.oo, chunks_per_tile=P.TC,
                                sync=self.sy)

    def replay_and_check(self):
        ref_bytes, ref_offs, ref_sync = self.ref
        self.out.zero_()
        self.oo.zero_()
        self.sy.fill_(0x5A5A5A5A)
        self.graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(self.oo.cpu().numpy().view(np.uint64), ref_offs)
        assert np.array_equal(self.out[:len(ref_bytes)].cpu().numpy(), ref_bytes)
        gs = self.sy.cpu().numpy().view(np.uint32)[:len(ref_sync)]
        assert np.array_equal(gs, ref_sync)  # (every tile of these batches is staged)


def test_captured_pack_replayed_between_other_packs():
    # a captured pack runs later and any number of times: it must not rely on
    # what the context knew about the workspace when it was captured
    ctx = _ctx()
    try:
        ctx.reserve(1 << 16)  # (before the capture: the workspace must not move)
        big = _plain(10, 200 * P.TC + 3)
        ref_big = P.check_pack(ctx, *big, True)  # the workspace is known clean from here
        cap = _Captured(ctx, *_plain(11, 120 * P.TC + 5))
        cap.replay_and_check()
        _check_messages(ctx, 12, 300)  # the gap pack leaves the workspace used
        cap.replay_and_check()
        P.check_pack(ctx, *big, True, ref=ref_big)
        ovf = _overflowing(13, 60 * P.TC)
        P.check_pack(ctx, *ovf, True)
        cap.replay_and_check()
        cap.replay_and_check()
        P.check_pack(ctx, *big, False, ref=ref_big)
    finally:
        ctx.close()


def test_pack_captured_over_used_workspace_is_not_taken_as_run():
    ctx = _ctx()
    try:
        ctx.reserve(1 << 16)
        _check_messages(ctx, 14, 300)  # leaves the workspace used
        cap = _Captured(ctx, *_plain(15, 90 * P.TC))  # captured, not run
        P.check_pack(ctx, *_plain(16, 150 * P.TC + 1), True)
        cap.replay_and_check()
        P.check_pack(ctx, *_plain(16, 150 * P.TC + 1), False)
    finally:
        ctx.close()
