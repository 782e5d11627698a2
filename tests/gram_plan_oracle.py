"""The rules that chose k_gram's launch variant before csrc/mcba_gram_plan.h, transcribed literally from derive_geometry, launch_gram,
gram_chunk_doubles and lm_reduce_chain as they stood in "refine_extrinsics for up to 64 cameras: a tiled Schur reduction": five rounds of
rules overwriting one another, in their order.  This is the reference of tests/test_hostcheck_gram_plan.py and deliberately not the shape of
the planner.  The transcription was compared with those four functions at that commit line by line (integer divisions, the strict and
non-strict bounds, the order of the overwrites, `gram_split != 3` in the round-4 block, the clamp of the forced code)."""


def parent_plan(C, nfb, N, slots, ps_ok, cw, force_split=None, force_npw=None):
    """derive_geometry: (split, npw, nchunk) as the handle kept them, None where it refused."""
    items = C * nfb
    split = int(items < 3 * slots // 4 or (slots < items <= 3 * slots // 2))
    npw, nchunk = 4, 0
    if items > 2 * slots and 0 < items % slots <= slots // 2: split = 2
    if items > slots:
        fba = ((items // slots) * slots // C) & ~3; tail = C * (nfb - fba)
        if fba > 0 and 0 < tail <= slots // 2 and N >= 128:
            nch = min(8, slots // tail, N // 8)
            if nch >= 2: split, nchunk = 3, nch
    if ps_ok:
        if items <= slots // 4: split, npw = 4, 4
        elif items <= slots // 2: split, npw = 4, 2
        elif items <= slots: split = 0
        else:
            fba = ((items // slots) * slots // C) & ~3; tail = C * (nfb - fba)
            if fba > 0 and 0 < tail <= slots // 4: split, npw = 5, 4
            elif fba > 0 and 0 < tail <= slots // 2 and split != 3: split, npw = 5, 2
    if force_split is not None:
        split = max(0, min(5, force_split))
        if split == 3 and nchunk < 2: nchunk = max(2, min(4, N // 8))
        if split >= 4 and not ps_ok: return None          # the refusal
    if force_npw is not None: npw = 2 if force_npw == 2 else 4
    if cw == 6 and split != 4: split = 1
    return split, npw, nchunk


def parent_head(C, nfb, slots):
    """The head / tail cut as launch_gram, gram_chunk_doubles and derive_geometry each wrote it."""
    return ((C * nfb // slots) * slots // C) & ~3


def parent_launch(C, nfb, slots, cw, split, nchunk):
    """launch_gram's fallbacks: (whole, tail) -- whole in 'fused', 'roles', 'psplit', 'role_a'; tail in None, 'roles', 'chunks', 'psplit'."""
    fba = parent_head(C, nfb, slots)
    if cw == 6:
        return ("psplit" if split == 4 else "role_a"), None
    if split == 4:
        return "psplit", None
    if split == 5:
        return "fused", ("psplit" if 0 < fba < nfb else None)
    if split == 1:
        return "roles", None
    if split == 3:
        return "fused", ("chunks" if 0 < fba < nfb and nchunk >= 2 else None)
    return "fused", ("roles" if split == 2 and 0 < fba < nfb else None)


def parent_chunk_doubles(C, nfb, nchunk, slots):
    """gram_chunk_doubles."""
    return C * (nfb - parent_head(C, nfb, slots)) * nchunk * 88 * 64


def parent_cost_slots(C, nfb, slots, split):
    """lm_reduce_chain: (cstride, cinner, cdense) of SyrkFuse."""
    if split == 4:
        return 4, nfb, 0
    fba = parent_head(C, nfb, slots)
    if split == 5 and 0 < fba < nfb:
        return 4, fba // 4 + nfb - fba, fba // 4
    return 4, (nfb + 3) // 4, 1 << 30
