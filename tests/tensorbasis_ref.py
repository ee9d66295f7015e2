"""Reference vector-Jacobian products of the tensor-basis operators, assembled from two parts that are each pinned to the CPU oracle:

  (a) `oracle.gradu` and `oracle.divoftensor_` are linear: their dense transposes are taken by unit probes (`dense_transpose_apply`, as in
      tests/test_gpu_adjoint.py);
  (b) the pointwise map (S, R) -> (B_1..B_nb, V_1..V_nv) is restated below with torch CPU float64 tensors (the expressions of
      `oracle.tensorbasis`), and torch.autograd gives its VJP.

tests/test_tensorclosure_cpu.py pins (b)∘gradu to `oracle.tensorbasis`.

Layouts.  Oracle: B is N + (nb, D, D) with [..., i, a, b], V is N + (nv,).  Library: B is N + (nb·D·D,) with element (a, b) of tensor i at
i·D·D + a + D·b; a symmetric tensor is N + (D(D+1)/2,) in the order [xx, yy, (zz), xy, (xz, yz)].  The cotangent of a symmetric tensor has
the same D(D+1)/2 fields, <taubar, tau> = Σ_{a<=b} taubar_ab tau_ab; `full_cotangent` is the D×D matrix with that inner product against a
symmetric matrix (off-diagonals halved on both sides)."""
import numpy as np
import torch


def sizes(D):
    """(nb, nv, ns)"""
    return ((3, 2) if D == 2 else (11, 5)) + (D * (D + 1) // 2,)


def sym_pairs(D):
    return [(0, 0), (1, 1), (0, 1)] if D == 2 else [(0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2)]


def full_from_sym(t):
    """N + (ns,) -> the symmetric N + (D, D) tensor it stores."""
    ns = t.shape[-1]
    D = 2 if ns == 3 else 3
    out = np.zeros(t.shape[:-1] + (D, D))
    for q, (a, b) in enumerate(sym_pairs(D)):
        out[..., a, b] = t[..., q]
        out[..., b, a] = t[..., q]
    return out


def full_cotangent(t):
    """N + (ns,) cotangent -> N + (D, D) with <full, B> = Σ_{a<=b} t_ab B_ab for symmetric B."""
    out = full_from_sym(t)
    D = out.shape[-1]
    for a in range(D):
        for b in range(D):
            if a != b:
                out[..., a, b] /= 2
    return out


def lib_B_from_oracle(B):
    """N + (nb, D, D) -> N + (nb·D·D,) in the library's field order."""
    return np.asfortranarray(np.swapaxes(B, -1, -2).reshape(B.shape[:-3] + (-1,)))


def oracle_B_from_lib(B, D):
    return np.swapaxes(B.reshape(B.shape[:-1] + (-1, D, D)), -1, -2)


def pointwise(G):
    """torch: G (..., D, D) -> (list of B_i (..., D, D), list of V_j (...)): the expressions of oracle.tensorbasis."""
    D = G.shape[-1]
    Gt = G.transpose(-1, -2)
    S = (G + Gt) / 2
    R = (G - Gt) / 2
    Id = torch.eye(D, dtype=G.dtype).expand(S.shape)

    def tr(X):
        return torch.diagonal(X, dim1=-2, dim2=-1).sum(-1)

    if D == 2:
        Bs = [Id, S, S @ R - R @ S]
        Vs = [(S * S).sum((-1, -2)), (R * R).sum((-1, -2))]
    else:
        Bs = [Id, S, S @ R - R @ S, S @ S, R @ R, S @ S @ R - R @ S @ S, S @ R @ R + R @ R @ S, R @ S @ R @ R - R @ R @ S @ R,
              S @ R @ S @ S - S @ S @ R @ S, S @ S @ R @ R + R @ R @ S @ S, R @ S @ S @ R @ R - R @ R @ S @ S @ R]
        Vs = [tr(S @ S), tr(R @ R), tr(S @ S @ S), tr(S @ R @ R), tr(S @ S @ R @ R)]
    return Bs, Vs


def _ip(so):
    return tuple(slice(lo, hi) for lo, hi in so.grid.Ip)


def forward(o, so, u):
    """(B, V) in the oracle's layout from oracle.gradu and `pointwise`."""
    g = so.grid
    Bs, Vs = pointwise(torch.from_numpy(np.ascontiguousarray(o.gradu(u, so))))
    N = tuple(g.N)
    B = np.zeros(N + (len(Bs), g.D, g.D))
    V = np.zeros(N + (len(Vs),))
    for i, b in enumerate(Bs):
        B[_ip(so) + (i,)] = b.numpy()
    for i, v in enumerate(Vs):
        V[_ip(so) + (i,)] = v.numpy()
    return B, V


def dense_transpose_apply(L, shape, w):
    """(dL)^T w of a linear map L on numpy fields of `shape`, by unit probes."""
    n = int(np.prod(shape))
    wf = w.reshape(-1, order="F")
    out = np.empty(n)
    e = np.zeros(n)
    for k in range(n):
        e[k] = 1.0
        out[k] = np.dot(wf, L(e.reshape(shape, order="F")).reshape(-1, order="F"))
        e[k] = 0.0
    return out.reshape(shape, order="F")


def gradu_transpose(o, so, Gbar):
    """ubar = (∇)ᵀ Gbar over the whole padded array; Gbar: Ip-shape + (D, D)."""
    g = so.grid
    return dense_transpose_apply(lambda x: o.gradu(x, so), tuple(g.N) + (g.D,), Gbar)


def tensorbasis_vjp(o, so, u, Bbar=None, Vbar=None):
    """ubar of (B, V) = tensorbasis(u) for cotangents in the oracle's layout (either may be None); they are read on Ip only."""
    G = torch.from_numpy(np.ascontiguousarray(o.gradu(u, so))).requires_grad_(True)
    Bs, Vs = pointwise(G)
    loss = 0.0
    if Bbar is not None:
        for i, b in enumerate(Bs):
            loss = loss + (torch.from_numpy(np.ascontiguousarray(Bbar[_ip(so) + (i,)])) * b).sum()
    if Vbar is not None:
        for i, v in enumerate(Vs):
            loss = loss + (torch.from_numpy(np.ascontiguousarray(Vbar[_ip(so) + (i,)])) * v).sum()
    (Gbar,) = torch.autograd.grad(loss, G)
    return gradu_transpose(o, so, Gbar.numpy())


def closure_vjp(o, so, u, a=None, taubar=None, Vbar=None):
    """(ubar, abar) of tau = Σ_i a_i B_i(u) (N + (ns,)) and V(u) for the cotangents taubar (N + (ns,)) and Vbar (N + (nv,)); `a` is
    N + (nb,).  abar is None when a is."""
    g = so.grid
    D = g.D
    G = torch.from_numpy(np.ascontiguousarray(o.gradu(u, so))).requires_grad_(True)
    Bs, Vs = pointwise(G)
    loss = 0.0
    at = None
    if a is not None:
        at = torch.from_numpy(np.ascontiguousarray(a[_ip(so)])).requires_grad_(True)
        tau = sum(at[..., i, None, None] * b for i, b in enumerate(Bs))
        tb = torch.from_numpy(np.ascontiguousarray(taubar[_ip(so)]))
        for q, (p, r) in enumerate(sym_pairs(D)):
            loss = loss + (tb[..., q] * tau[..., p, r]).sum()
    if Vbar is not None:
        for i, v in enumerate(Vs):
            loss = loss + (torch.from_numpy(np.ascontiguousarray(Vbar[_ip(so) + (i,)])) * v).sum()
    grads = torch.autograd.grad(loss, (G,) + ((at,) if at is not None else ()))
    ubar = gradu_transpose(o, so, grads[0].numpy())
    abar = None
    if at is not None:
        abar = np.zeros(tuple(g.N) + (len(Bs),))
        abar[_ip(so)] = grads[1].numpy()
    return ubar, abar


def divoftensor_sym(o, so, t):
    """This library's divoftensor on the D(D+1)/2 symmetric fields, through the oracle's full-tensor operator."""
    g = so.grid
    return o.divoftensor_(np.zeros(tuple(g.N) + (g.D,), order="F"), full_from_sym(t), so)


def divoftensor_transpose(o, so, sbar):
    g = so.grid
    return dense_transpose_apply(lambda x: divoftensor_sym(o, so, x), tuple(g.N) + (sizes(g.D)[2],), sbar)


def relmax(a, b):
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300))
