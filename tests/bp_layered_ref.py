"""TEST INFRASTRUCTURE ONLY -- NumPy restatement of the layered (row-serial)
BP schedule (DESIGN.md "Layered schedule"), the oracle of bp_layered.hip.

The graph is in the reference layout (vdeg, cdeg, intrlv); layer l is the
checks [l S, (l + 1) S).  Per codeword app starts as ch and one message R[e]
per edge, in check-ordered message order, starts at 0.  An iteration takes the
layers in ascending order; a check c with ports k on variables v_k does

    Q_k = app[v_k] - R[c,k]
    R'[c,.] = Lxfb(Q)              (c_ldpc.c:294-314, forward / backward)
    app[v_k] = Q_k + R'[c,k];  R[c,k] = R'[c,k]

with Lxfb's pairwise operation Lxor (c_ldpc.c:234-251) without correction and
every output times `corr` for min-sum, with the plain log(1 + exp(.))
correction for sumprod2.  After the last layer the syndrome of the hard
decisions app < 0 over all checks stops a codeword; `it` is the 0-based index
of that iteration, else max_it, and app is as the last executed layer left
it.  The checks of a layer touch disjoint variables, so they are evaluated
side by side (vectorised over the layer and the batch); within a check every
operation is in the order above, in `dtype` throughout, which makes the
float32 form a bit-for-bit model of the float32 min-sum kernel."""
import numpy as np


def lxor(a, b, corr, dtype):
    """Lxor (c_ldpc.c:234-251) elementwise in dtype."""
    same = np.signbit(a) == np.signbit(b)
    out = np.where(same, dtype(1), dtype(-1)) * np.fmin(np.abs(a), np.abs(b))
    if corr:
        out = out + np.log(dtype(1) + np.exp(-np.abs(a + b)))
        out = out - np.log(dtype(1) + np.exp(-np.abs(a - b)))
    return out.astype(dtype, copy=False)


def lxfb(Q, corr, dtype):
    """Lxfb (c_ldpc.c:294-314) over the ports Q[0..dc-1] (arrays of one
    shape): the extrinsic outputs, port by port."""
    dc = len(Q)
    f, b = [None] * dc, [None] * dc
    f[0] = Q[0]
    b[dc - 1] = Q[dc - 1]
    for i in range(1, dc):
        f[i] = lxor(f[i - 1], Q[i], corr, dtype)
        b[dc - 1 - i] = lxor(b[dc - i], Q[dc - 1 - i], corr, dtype)
    out = [None] * dc
    out[0] = b[1]
    out[dc - 1] = f[dc - 2]
    for i in range(1, dc - 1):
        out[i] = lxor(f[i - 1], b[i + 1], corr, dtype)
    return out


def edge_variables(vdeg, cdeg, intrlv):
    """(coff, mvar): message offset of every check and the variable of every
    check-ordered message."""
    vdeg, cdeg, intrlv = (np.asarray(a, dtype=np.int64) for a in (vdeg, cdeg, intrlv))
    mvar = np.empty(len(intrlv), np.int64)
    mvar[intrlv] = np.repeat(np.arange(len(vdeg)), vdeg)
    return np.concatenate([[0], np.cumsum(cdeg)]), mvar


def layer_ok(vdeg, cdeg, intrlv, layer):
    """layer divides Nc and no variable occurs twice within a layer."""
    coff, mvar = edge_variables(vdeg, cdeg, intrlv)
    nc = len(cdeg)
    if layer <= 0 or nc % layer:
        return False
    for l in range(nc // layer):
        v = mvar[coff[l * layer]:coff[(l + 1) * layer]]
        if len(np.unique(v)) != len(v):
            return False
    return True


def layered(vdeg, cdeg, intrlv, ch, layer, max_it, dectype, corr=0.7, dtype=np.float64):
    """Layered decode of a [B, N] batch (or one [N] vector) of channel LLRs.
    Returns (app dtype[B, N], it int32[B])."""
    if dectype not in ("minsum", "sumprod2"):
        raise ValueError("the layered schedule decodes minsum and sumprod2")
    if max_it < 1:
        raise ValueError("max_it < 1")
    if not layer_ok(vdeg, cdeg, intrlv, layer):
        raise ValueError("invalid layer size")
    dtype = np.dtype(dtype).type
    single = np.ndim(ch) == 1
    app = np.array(np.atleast_2d(ch), dtype=dtype)  # (a copy: app starts as ch)
    cdeg = np.asarray(cdeg, dtype=np.int64)
    coff, mvar = edge_variables(vdeg, cdeg, intrlv)
    B, nc = app.shape[0], len(cdeg)
    R = np.zeros((B, len(mvar)), dtype)
    factor = dtype(corr)
    use_corr = dectype == "sumprod2"
    # the checks of a layer by degree: (message index of port k, variable of port k) for k < dc
    groups = []
    for l in range(nc // layer):
        c = np.arange(l * layer, (l + 1) * layer)
        g = []
        for dc in np.unique(cdeg[c]):
            cc = c[cdeg[c] == dc]
            msg = [coff[cc] + k for k in range(int(dc))]
            g.append((msg, [mvar[m] for m in msg]))
        groups.append(g)
    its = np.full(B, max_it, np.int32)
    live = np.arange(B)
    with np.errstate(over="ignore"):
        for it in range(max_it):
            a, r = app[live], R[live]
            for g in groups:
                for msg, var in g:
                    Q = [a[:, v] - r[:, m] for m, v in zip(msg, var)]
                    out = lxfb(Q, use_corr, dtype)
                    for k, (m, v) in enumerate(zip(msg, var)):
                        o = out[k] if use_corr else out[k] * factor
                        r[:, m] = o
                        a[:, v] = Q[k] + o
            app[live], R[live] = a, r
            par = np.add.reduceat((a[:, mvar] < 0).astype(np.int64), coff[:-1], axis=1)
            done = ~(par & 1).any(axis=1)
            its[live[done]] = it
            live = live[~done]
            if not len(live):
                break
    return (app[0], int(its[0])) if single else (app, its)
