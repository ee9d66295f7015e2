"""numpy restatement of the DNS-to-LES filters, written from the index formulas, for the filter tests.

Fields are the padded arrays (N per direction, ghosts included, component last); indices 0-based.  `Iu` is the coarse grid's
`Iu[α][β] = (lo, hi)` half-open ranges; `n_les` / `n_dns` are interior volumes per direction.

  face    v[I, α] = mean u[f, α],  f_α = lo_α + comp·(I_α − lo_α) + comp − 1,  f_β = lo_β + comp·(I_β − lo_β) + (0..comp−1)
  volume  v[I, α] = mean u[f, α],  f_α = comp·I_α − h .. comp·I_α + h  (h = comp // 2; comp + 1 planes for even comp, comp for odd),
          f_β = comp·(I_β − 1) + (1..comp), every f wrapped into the fine interior 1..n_dns   (all-periodic grids: lo = 1)
  reconstruct  u[f, α] = ((comp − i_α)·v[c, α] + i_α·v[c − e_α, α]) / comp,  c = ceil(f / comp),  i = comp·c − f,  c − e_α wrapped
  pullbacks    ubar[f, α] += w[I, α] / count for every (I, f) pair of the two averages above: scatters over the same index tuples
"""
import itertools

import numpy as np


def subdivide(x, comp):
    """Fine face coordinates: every interval of `x` split into `comp` equal parts (nested: fine[comp·i] == x[i] exactly)."""
    x = np.asarray(x, dtype=np.float64)
    out = [x[0]]
    for a, b in zip(x[:-1], x[1:]):
        out.extend(a + (b - a) * q / comp for q in range(1, comp))
        out.append(b)
    return np.array(out)


def face_average(u, Iu, shape_les, comp, out=None):
    D = u.shape[-1]
    v = np.zeros(tuple(shape_les) + (D,), order="F") if out is None else out
    for a in range(D):
        lo = [Iu[a][b][0] for b in range(D)]
        hi = [Iu[a][b][1] for b in range(D)]
        sl = tuple(slice(lo[b], hi[b]) for b in range(D))
        acc = np.zeros([hi[b] - lo[b] for b in range(D)])
        windows = [[comp - 1] if b == a else range(comp) for b in range(D)]
        for off in itertools.product(*windows):
            idx = tuple(lo[b] + comp * (np.arange(lo[b], hi[b]) - lo[b]) + off[b] for b in range(D))
            acc += u[..., a][np.ix_(*idx)]
        v[sl + (a,)] = acc / comp ** (D - 1)
    return v


def volume_average(u, n_les, comp, out=None):
    D = u.shape[-1]
    v = np.zeros(tuple(n + 2 for n in n_les) + (D,), order="F") if out is None else out
    h = comp // 2
    nplane = comp + 1 if comp % 2 == 0 else comp
    for a in range(D):
        acc = np.zeros(n_les)
        windows = [range(-h, -h + nplane) if b == a else range(1 - comp, 1) for b in range(D)]
        for off in itertools.product(*windows):
            idx = tuple((comp * np.arange(1, n_les[b] + 1) + off[b] - 1) % (comp * n_les[b]) + 1 for b in range(D))
            acc += u[..., a][np.ix_(*idx)]
        v[tuple(slice(1, n + 1) for n in n_les) + (a,)] = acc / (nplane * comp ** (D - 1))
    return v


def face_average_pullback(w, Iu, shape_dns, comp):
    """ubar = Φᵀ w over the whole padded fine array: every coarse cotangent scattered to the index tuples `face_average` reads."""
    D = w.shape[-1]
    ubar = np.zeros(tuple(shape_dns) + (D,), order="F")
    for a in range(D):
        lo = [Iu[a][b][0] for b in range(D)]
        hi = [Iu[a][b][1] for b in range(D)]
        sl = tuple(slice(lo[b], hi[b]) for b in range(D))
        share = w[sl + (a,)] / comp ** (D - 1)
        windows = [[comp - 1] if b == a else range(comp) for b in range(D)]
        for off in itertools.product(*windows):
            idx = tuple(lo[b] + comp * (np.arange(lo[b], hi[b]) - lo[b]) + off[b] for b in range(D))
            np.add.at(ubar[..., a], np.ix_(*idx), share)
    return ubar


def volume_average_pullback(w, n_les, comp):
    """ubar = Φᵀ w over the whole padded fine array (all-periodic grids): the scatter over the wrapped index tuples of `volume_average`."""
    D = w.shape[-1]
    ubar = np.zeros(tuple(comp * n + 2 for n in n_les) + (D,), order="F")
    h = comp // 2
    nplane = comp + 1 if comp % 2 == 0 else comp
    for a in range(D):
        share = w[tuple(slice(1, n + 1) for n in n_les) + (a,)] / (nplane * comp ** (D - 1))
        windows = [range(-h, -h + nplane) if b == a else range(1 - comp, 1) for b in range(D)]
        for off in itertools.product(*windows):
            idx = tuple((comp * np.arange(1, n_les[b] + 1) + off[b] - 1) % (comp * n_les[b]) + 1 for b in range(D))
            np.add.at(ubar[..., a], np.ix_(*idx), share)
    return ubar


def reconstruct(v, n_les, comp, out=None):
    D = v.shape[-1]
    n_dns = [comp * n for n in n_les]
    u = np.zeros(tuple(n + 2 for n in n_dns) + (D,), order="F") if out is None else out
    f = [np.arange(1, n + 1) for n in n_dns]
    c = [(fi + comp - 1) // comp for fi in f]
    for a in range(D):
        i = comp * c[a] - f[a]
        left = list(c)
        left[a] = np.where(c[a] == 1, n_les[a], c[a] - 1)
        shape = [1] * D
        shape[a] = -1
        w = i.reshape(shape)
        val = ((comp - w) * v[..., a][np.ix_(*c)] + w * v[..., a][np.ix_(*left)]) / comp
        u[tuple(slice(1, n + 1) for n in n_dns) + (a,)] = val
    return u
