"""Phrase assembly restated in numpy float64 (the definition: include/goofer_hip.h, goofer_phrase_note), one loop per note.

    track[t] = sum_i g_i(u) * x_i[skip_i + u],  u = t - start_i,  over the notes with 0 <= u < take_i and skip_i + u < len_i
    g = val[k] + (val[k+1] - val[k]) * ((u - pos[k]) / (pos[k+1] - pos[k])),  k the largest index with pos[k] <= u

``mix`` also returns, per track sample, B = sum_i max_k |val_i[k]| * |x_i| and the cover depth D (how many notes reach it):
what the error bound of the fp32 kernel is made of, |got - ref| <= (8 + D) * 2^-24 * B — six roundings in the gain, one in the
product, D in the sum.  ``cover`` is the cover table by brute force."""
import numpy as np

TILE = 2048


def effective(note, length, total_out):
    """[lo, hi) of the track that the note reaches (empty: lo >= hi)"""
    eff = min(int(note["take"]), int(length) - int(note["skip"]))
    if eff <= 0:
        return 0, 0
    return max(int(note["start"]), 0), min(int(note["start"]) + eff, int(total_out))


def mix(xs, notes, total_out):
    """xs: the notes' samples (list of arrays); notes: records with start / skip / take / pos / val.  (track, B, D), float64 /
    float64 / int64 [total_out]."""
    track = np.zeros(total_out, dtype=np.float64)
    B = np.zeros(total_out, dtype=np.float64)
    D = np.zeros(total_out, dtype=np.int64)
    for x, r in zip(xs, notes):
        x = np.asarray(x, dtype=np.float64)
        start, skip, take = int(r["start"]), int(r["skip"]), int(r["take"])
        pos, val = np.asarray(r["pos"], dtype=np.float64), np.asarray(r["val"], dtype=np.float64)
        eff = min(take, len(x) - skip)
        if eff <= 0:
            continue
        u = np.arange(eff, dtype=np.int64)
        t = start + u
        keep = (t >= 0) & (t < total_out)
        u, t = u[keep], t[keep]
        if not len(u):
            continue
        uf = u.astype(np.float64)
        k = np.searchsorted(pos, uf, side="right") - 1            # the largest k with pos[k] <= u; pos[6] = take > u: k <= 5
        assert k.min() >= 0 and k.max() <= 5
        g = val[k] + (val[k + 1] - val[k]) * ((uf - pos[k]) / (pos[k + 1] - pos[k]))
        xi = x[skip + u]
        track[t] += g * xi
        B[t] += np.abs(val).max() * np.abs(xi)
        D[t] += 1
    return track, B, D


def bound(B, D):
    return (8.0 + D) * 2.0 ** -24 * B


def cover(notes, lengths, total_out):
    """(tile_off, tile_notes) by brute force: every tile against every note"""
    tiles = (total_out + TILE - 1) // TILE
    off, lst = [0], []
    for t in range(tiles):
        for i, (r, n) in enumerate(zip(notes, lengths)):
            lo, hi = effective(r, n, total_out)
            if lo < hi and lo < (t + 1) * TILE and hi > t * TILE:
                lst.append(i)
        off.append(len(lst))
    return np.array(off, dtype=np.int64), np.array(lst, dtype=np.int32)
