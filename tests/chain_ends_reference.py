"""The reported energy of a structured anneal, restated in plain float64 loops ("Chain ends";
csrc/mi_sa_chain_ends.h).  TEST INFRASTRUCTURE ONLY.

From the states a run returned and the model AS THE DEVICE HOLDS IT -- the CSR in stored order, in seat space for a padded
layout (lin = +inf at a hole of a binary model, ``present`` false at a hole of a Potts model), the coefficients in the
precision the device sums them in (the fp32 model's values, or the fp64 energy model's) -- these functions reproduce the
reported energy BIT FOR BIT: the lanes' partial sums in the kernels' order, the xor butterfly over the 64 lanes, the
one closing expression.  Python floats are IEEE doubles; nothing here sums with numpy, extended precision or an fma.

Padding entries of the device's slot-ELL rows add +0.0 to a sum that started at +0.0, which changes nothing, so the CSR
rows suffice."""
import numpy as np

LANES = 64


def butterfly(v):
    """wave_sum_f64: v[l] += v[l ^ off] on every lane at once, off = 32, 16, ... 1.  Returns lane 0's value (every lane ends
    with the same bits: the two operands of each addition are swapped between the partner lanes)."""
    v = [float(x) for x in v]
    assert len(v) == LANES
    off = 32
    while off:
        v = [v[l] + v[l ^ off] for l in range(LANES)]
        off >>= 1
    return v[0]


def binary_energy(x, rowptr, col, val, lin, c_pair, offset=0.0, weights=None, waves=1):
    """Reported energy of one replica of the binary family (K2, K2s, K2w, K2p).

    x: states in device order [n_dev]; val / lin: float32 arrays (the fp32 model) or float64 ones (an fp64 energy model),
    c_pair to match; weights: integer pair-term weights per device position (None: all 1); waves: wavefronts per replica
    (K2s with 2 or 4: wave w sums the slots w, w + waves, ... and the waves' sums are added in ascending order)."""
    x = np.asarray(x)
    n_dev = len(x)
    slots = -(-n_dev // LANES)
    slots += (-slots) % waves
    wave_sums = []
    for w in range(waves):
        lane_e = []
        for lane in range(LANES):
            e = 0.0
            for t in range(w, slots, waves):
                i = t * LANES + lane
                if i >= n_dev or not x[i]:
                    continue
                acc = 0.0
                for k in range(rowptr[i], rowptr[i + 1]):
                    if x[col[k]]:
                        acc += float(val[k])
                e += float(lin[i]) + 0.5 * acc
            lane_e.append(e)
        wave_sums.append(butterfly(lane_e))
    if waves == 1:
        e = wave_sums[0]
    else:
        e = 0.0
        for s in wave_sums:
            e += s
    cnt = cnt2 = 0                                                   # exact integers on the device too
    for i in range(n_dev):
        if x[i]:
            wi = 1 if weights is None else int(weights[i])
            cnt += wi
            cnt2 += wi * wi
    return e + float(c_pair) * 0.5 * (float(cnt) * float(cnt) - float(cnt2)) + float(offset)


def binary_energies(X, *args, **kw):
    return np.array([binary_energy(x, *args, **kw) for x in np.asarray(X)], dtype=np.float64)


def potts_energy(lab, rowptr, col, val, c_pair, offset, K, present=None, nw64=None):
    """Reported energy of one replica of the Potts family (K3, K3f).

    lab: labels in device order [n_dev] (0 at a hole); present: False at the holes of a padded layout (None: none);
    nw64: the fp64 node weights per device position (0 at a hole) of a model with node weights -- c_pair and offset are
    then the replica's resolution group's; None: the uniform pair term."""
    lab = np.asarray(lab)
    n_dev = len(lab)
    slots = -(-n_dev // LANES)
    cp = float(c_pair)
    lane_e = []
    for lane in range(LANES):
        e = 0.0
        for t in range(slots):
            i = t * LANES + lane
            if i >= n_dev:
                continue
            for k in range(rowptr[i], rowptr[i + 1]):
                if col[k] > i and lab[col[k]] == lab[i]:
                    e += float(val[k])
        lane_e.append(e)
    if nw64 is None:
        for q in range(min(K, LANES)):                               # lane q carries cluster q's pairs
            cnt = 0
            for i in range(n_dev):
                if lab[i] == q and (present is None or present[i]):
                    cnt += 1
            lane_e[q] += cp * 0.5 * float(cnt) * float(cnt - 1)
    else:
        own = []
        for lane in range(LANES):
            o = 0.0
            for t in range(slots):
                i = t * LANES + lane
                w = float(nw64[i]) if i < n_dev else 0.0
                o -= w * w
            own.append(o)
        tot = 0.0
        for q in range(K):
            s = []
            for lane in range(LANES):
                sl = 0.0
                for t in range(slots):
                    i = t * LANES + lane
                    if i < n_dev and lab[i] == q:
                        sl += float(nw64[i])
                s.append(sl)
            W = butterfly(s)
            tot += W * W
        for lane in range(LANES):
            lane_e[lane] += 0.5 * cp * (own[lane] + (tot if lane == 0 else 0.0))
    return butterfly(lane_e) + float(offset)


def potts_energies(L, *args, **kw):
    return np.array([potts_energy(l, *args, **kw) for l in np.asarray(L)], dtype=np.float64)
