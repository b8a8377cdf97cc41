"""The compaction policy of the per-layer layered decoder (include/ibldpc.h "Layered min-sum", compaction) restated
in Python, independent of csrc/layered_plan.h: from the reference's per-codeword iteration counts it lists the
compactions a decode makes and follows the columns through them."""
import numpy as np

TILE = 64


def wanted(R, E, pct):
    """R running codewords in an extent of E columns: compact iff R > 0 and the move frees at least
    max(1, ceil(pct tE / 100)) of the extent's tE tiles."""
    tE, tR = -(-E // TILE), -(-R // TILE)
    return R > 0 and tE - tR >= max(1, -(-pct * tE // 100))


def compactions(iters, B, imax, every, pct, early_stop=True):
    """``iters``: the reference's iteration count of each of the B codewords (imax: never finished by the stop
    check, which runs after iterations 1 .. imax - 1). Returns ``(events, extent, orig)``: the list of
    ``(iteration, E, R)`` compactions, the extent at the end, and ``orig`` [extent], the caller's column of the
    codeword in each column still in use."""
    iters = np.asarray(iters)[:B]
    orig = np.arange(B)
    events = []
    if early_stop:
        for it in range(1, imax):
            if it % every:
                continue
            running = iters[orig] > it      # finished by the stop check of iteration it or earlier: not running
            R, E = int(running.sum()), len(orig)
            if wanted(R, E, pct):
                events.append((it, E, R))
                orig = orig[running]        # stable: the running columns keep their order
    return events, len(orig), orig
