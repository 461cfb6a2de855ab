"""Shared by the chunk-step pack tests: one device pack through the context
API compared byte for byte with the oracle (bytes, offsets, sync index)."""
import numpy as np

import oracle_lib as O

TC = 16                # chunks per tile of pack_cs_kernel
STEP_WORDS = 128       # a chunk longer than a step leaves its tile unstaged
STAGE_BYTES = 4 * 4192  # and so does a tile whose packed bytes pass its staging regions
SYNC_NONE = 0xFFFFFFFF


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).cuda()


def oracle(words, offs):
    """(packed bytes, byte offsets, sync index) of the batch."""
    st, ref, ref_offs = O.pack_batch(words, offs)
    assert st == 0
    return ref, ref_offs, O.sync_index(ref, ref_offs, offs)


def unstaged_tiles(offs, ref_offs, tc=TC):
    """Tiles of a chunk-step pack that take the streaming path."""
    n = len(offs) - 1
    out = []
    for t in range(-(-n // tc)):
        c0, c1 = t * tc, min(t * tc + tc, n)
        long_ = bool((np.diff(offs[c0:c1 + 1].astype(np.int64)) > STEP_WORDS).any())
        if long_ or int(ref_offs[c1]) - int(ref_offs[c0]) > STAGE_BYTES:
            out.append(t)
    return out


def expected_index(offs, ref_offs, ref_sync, tc=TC):
    """The oracle's index with the windows of the unstaged tiles left unprovided:
    entries [ceil(TW0 / 8), ceil(TW1 / 8)) of a tile of words [TW0, TW1)."""
    n = len(offs) - 1
    sw = O.sync_words()
    exp = ref_sync.copy()
    for t in unstaged_tiles(offs, ref_offs, tc):
        a, b = int(offs[t * tc]), int(offs[min(t * tc + tc, n)])
        exp[-(-a // sw):-(-b // sw)] = SYNC_NONE
    return exp


def check_pack(ctx, words, offs, sync, ref=None, chunks_per_tile=TC, exact_index=False):
    """Packs on the device and compares with the oracle; returns the oracle's
    triple so that callers packing the same batch again share it."""
    import torch
    if ref is None:
        ref = oracle(words, offs)
    ref_bytes, ref_offs, ref_sync = ref
    n, total = len(offs) - 1, int(offs[-1])
    out = torch.empty(ctx.batch_bound_bytes(total, n), dtype=torch.uint8, device="cuda")
    oo = torch.empty(n + 1, dtype=torch.int64, device="cuda")
    sy = torch.full((max(ctx.sync_entries(total), 1),), 0x5A5A5A5A, dtype=torch.int32,
                    device="cuda")
    ctx.pack_batch_into(dev(words), dev(offs), out, oo, chunks_per_tile=chunks_per_tile,
                        sync=sy if sync else None)
    torch.cuda.synchronize()
    got_offs = oo.cpu().numpy().view(np.uint64)
    assert np.array_equal(got_offs, ref_offs), np.nonzero(got_offs != ref_offs)[0][:8]
    got = out[:len(ref_bytes)].cpu().numpy()
    if not np.array_equal(got, ref_bytes):
        bad = int(np.nonzero(got != ref_bytes)[0][0])
        c = int(np.searchsorted(ref_offs, bad, side="right") - 1)
        raise AssertionError(f"bytes differ at {bad} (chunk {c})")
    if sync:
        gs = sy.cpu().numpy().view(np.uint32)[:len(ref_sync)]
        if exact_index:
            exp = expected_index(offs, ref_offs, ref_sync, chunks_per_tile)
            bad = np.nonzero(gs != exp)[0]
            assert len(bad) == 0, (bad[:8], gs[bad[:8]], exp[bad[:8]])
        else:
            provided = gs != SYNC_NONE
            assert np.array_equal(gs[provided], ref_sync[provided])
    return ref
