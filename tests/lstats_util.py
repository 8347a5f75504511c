"""numpy restatements of csrc/lstats.hip in the order include/evacx.h states: the rows' float32
arithmetic, the octave bucket, the 256-row block tree with its ascending block adds, the value
probe's float64 recurrence and the reduce's strided-then-pairwise order. tests/test_lstats_cpu.py
pins these on hand-made cases; tests/test_lstats_gpu.py compares the kernels with them bit for bit."""
import numpy as np

from span_reduce_util import SPAN, span_sum  # noqa: F401  (the reduce's order, shared with the other families' tests)

MAX_A, TD_BUCKETS, BLOCK = 8, 48, 256
I64 = ("steps", "steps_bad", "rows", "rows_bad", "n_done", "n_greedy", "n_clipped")
SUMS = ("s_q", "s_qmax", "s_y", "s_d", "s_absd", "s_d2", "s_rew", "s_loss", "s_norm")
EXT = ("max_absd", "max_q", "min_q", "max_loss", "max_norm")
F32 = np.float32


def first_max(M):
    """(value, index) of each row's first maximum: strict > while scanning j = 1..A-1."""
    M = np.asarray(M, F32)
    v, j = M[:, 0].copy(), np.zeros(len(M), np.int64)
    for k in range(1, M.shape[1]):
        up = M[:, k] > v
        v[up], j[up] = M[up, k], k
    return v, j


def first_min(M):
    M = np.asarray(M, F32)
    v = M[:, 0].copy()
    for k in range(1, M.shape[1]):
        up = M[:, k] < v
        v[up] = M[up, k]
    return v


def rows(Q, Qt, act, rew, done, gamma, sel=None, gamma_row=None):
    """One net's rows through the header's expressions, all float32: dict of a, q, qmax, jmax, qmin, y, d, bad."""
    Q, Qt, rew = np.asarray(Q, F32), np.asarray(Qt, F32), np.asarray(rew, F32)
    B, A = Q.shape
    i = np.arange(B)
    a = np.clip(np.asarray(act, np.int64), 0, A - 1)
    q = Q[i, a]
    qmax, jmax = first_max(Q)
    tv = Qt[i, np.clip(np.asarray(sel, np.int64), 0, A - 1)] if sel is not None else first_max(Qt)[0]
    gm = np.asarray(gamma_row, F32) if gamma_row is not None else np.full(B, gamma, F32)
    nd = np.where(np.asarray(done) != 0, F32(0), F32(1))
    with np.errstate(all="ignore"):
        y = rew + (gm * tv) * nd
        d = q - y
    assert y.dtype == F32 and d.dtype == F32
    bad = ~(np.isfinite(q) & np.isfinite(qmax) & np.isfinite(y))
    return dict(a=a, q=q, qmax=qmax, jmax=jmax, qmin=first_min(Q), y=y, d=d, bad=bad)


def bucket(absd):
    """k = min(max((bits(|d|) >> 23) - 103, 0), 47) of float32 values."""
    bits = np.asarray(absd, F32).reshape(-1).view(np.uint32).astype(np.int64)
    return np.clip((bits >> 23) - 103, 0, TD_BUCKETS - 1)


def block_sum(vals):
    """The step total of one net's per-row float64 values: 256-row blocks, s[t] = s[t] + s[t + h] for
    h = 128 .. 1 within a block, the block sums added in ascending order onto 0.0."""
    vals = np.asarray(vals, np.float64)
    nb = (len(vals) + BLOCK - 1) // BLOCK
    s = np.zeros(nb * BLOCK)
    s[:len(vals)] = vals
    s = s.reshape(nb, BLOCK).copy()
    h = BLOCK // 2
    with np.errstate(all="ignore"):
        while h:
            s[:, :h] = s[:, :h] + s[:, h:2 * h]
            h //= 2
        tot = np.float64(0.0)
        for b in range(nb):
            tot = tot + s[b, 0]
    return tot


def empty_window():
    w = {k: 0 for k in I64}
    w.update({k: np.float64(0.0) for k in SUMS})
    w.update(max_absd=-np.inf, max_q=-np.inf, min_q=np.inf, max_loss=-np.inf, max_norm=-np.inf)
    w["act_hist"], w["td_hist"] = np.zeros(MAX_A, np.int64), np.zeros(TD_BUCKETS, np.int64)
    return w


def fold(w, Q, Qt, act, rew, done, gamma, sel=None, gamma_row=None, loss=None, norm=None, max_norm=0.0):
    """evx_lstats_update of one net into the window dict w (in place); returns d_out (NaN on bad rows)."""
    r = rows(Q, Qt, act, rew, done, gamma, sel, gamma_row)
    good = ~r["bad"]
    f64 = {k: np.where(good, r[k].astype(np.float64), 0.0) for k in ("q", "qmax", "y", "d")}
    rew64 = np.where(good, np.asarray(rew, F32).astype(np.float64), 0.0)
    absd = np.abs(r["d"])
    with np.errstate(all="ignore"):
        for key, v in (("s_q", f64["q"]), ("s_qmax", f64["qmax"]), ("s_y", f64["y"]), ("s_d", f64["d"]),
                       ("s_absd", np.where(good, absd.astype(np.float64), 0.0)), ("s_d2", f64["d"] * f64["d"]),
                       ("s_rew", rew64)):
            w[key] = w[key] + block_sum(v)
    w["rows"] += len(good)
    w["rows_bad"] += int(r["bad"].sum())
    w["n_done"] += int((np.asarray(done)[good] != 0).sum())
    w["n_greedy"] += int((np.asarray(act, np.int64)[good] == r["jmax"][good]).sum())
    w["act_hist"] += np.bincount(r["a"][good], minlength=MAX_A)
    w["td_hist"] += np.bincount(bucket(absd[good]), minlength=TD_BUCKETS)
    if good.any():
        w["max_absd"] = max(w["max_absd"], float(absd[good].max()))
        w["max_q"] = max(w["max_q"], float(r["qmax"][good].max()))
        w["min_q"] = min(w["min_q"], float(r["qmin"][good].min()))
    w["steps"] += 1
    l32, n32 = (None if v is None else F32(v) for v in (loss, norm))
    if all(v is None or np.isfinite(v) for v in (l32, n32)):
        if l32 is not None:
            w["s_loss"] = w["s_loss"] + np.float64(l32)
            w["max_loss"] = max(w["max_loss"], float(l32))
        if n32 is not None:
            w["s_norm"] = w["s_norm"] + np.float64(n32)
            w["max_norm"] = max(w["max_norm"], float(n32))
            w["n_clipped"] += int(max_norm > 0 and n32 > F32(max_norm))
    else:
        w["steps_bad"] += 1
    return np.where(r["bad"], F32(np.nan), r["d"]).astype(F32)


# ------------------------------------------------------------------ the value probe
VP_FIELDS = ("open", "q0", "g", "disc", "len", "w_n", "w_bad", "w_q", "w_g", "w_e", "w_e2", "w_q2", "w_g2", "w_qg",
             "w_emin", "w_emax")


def probe_state(E):
    st = {k: np.zeros(E, np.float64) for k in VP_FIELDS}
    st["open"], st["len"] = np.zeros(E, np.uint8), np.zeros(E, np.int32)
    st["w_n"], st["w_bad"] = np.zeros(E, np.int64), np.zeros(E, np.int64)
    st["disc"][:] = 1.0
    st["w_emin"][:], st["w_emax"][:] = np.inf, -np.inf
    return st


def probe_step(st, Q, act, reward, done, gamma, R, lo=0, n=None):
    """evx_vprobe_update of envs [lo, lo + n) of the state st, in place: a float64 loop over envs.
    Q [n R][A] float32, act [n R], reward [n] float64, done [n]."""
    Q = np.asarray(Q, F32)
    A = Q.shape[1]
    n = len(reward) if n is None else n
    gamma = np.float64(gamma)
    with np.errstate(all="ignore"):
        for k in range(n):
            e = lo + k
            if not st["open"][e]:
                s = np.float64(0.0)
                for r in range(R):
                    s = s + np.float64(Q[k * R + r, min(max(int(act[k * R + r]), 0), A - 1)])
                st["q0"][e], st["g"][e], st["disc"][e], st["len"][e], st["open"][e] = s / np.float64(R), 0.0, 1.0, 0, 1
            st["g"][e] = st["g"][e] + st["disc"][e] * np.float64(reward[k])
            st["disc"][e] = st["disc"][e] * gamma
            st["len"][e] += 1
            if done[k]:
                q0, g = st["q0"][e], st["g"][e]
                if not np.isfinite(q0):
                    st["w_bad"][e] += 1
                else:
                    err = q0 - g
                    st["w_n"][e] += 1
                    for key, v in (("w_q", q0), ("w_g", g), ("w_e", err), ("w_e2", err * err), ("w_q2", q0 * q0),
                                   ("w_g2", g * g), ("w_qg", q0 * g)):
                        st[key][e] = st[key][e] + v
                    st["w_emin"][e] = min(st["w_emin"][e], err)
                    st["w_emax"][e] = max(st["w_emax"][e], err)
                st["open"][e] = 0


def probe_step_vec(st, Q, act, reward, done, gamma, R, lo=0, n=None):
    """probe_step with the envs as numpy lanes: the same float64 operations in the same order per env
    (tests/test_lstats_cpu.py holds it to the loop)."""
    Q = np.asarray(Q, F32)
    A = Q.shape[1]
    n = len(reward) if n is None else n
    sl = slice(lo, lo + n)
    a = np.clip(np.asarray(act, np.int64), 0, A - 1).reshape(n, R)
    qa = Q[np.arange(n * R), a.reshape(-1)].astype(np.float64).reshape(n, R)
    done = np.asarray(done).reshape(-1) != 0
    with np.errstate(all="ignore"):
        s = np.zeros(n)
        for r in range(R):
            s = s + qa[:, r]
        new = st["open"][sl] == 0
        st["q0"][sl] = np.where(new, s / np.float64(R), st["q0"][sl])
        g = np.where(new, 0.0, st["g"][sl])
        disc = np.where(new, 1.0, st["disc"][sl])
        st["len"][sl] = np.where(new, 0, st["len"][sl]) + 1
        g = g + disc * np.asarray(reward, np.float64)
        st["g"][sl], st["disc"][sl] = g, disc * np.float64(gamma)
        q0 = st["q0"][sl]
        fin = np.isfinite(q0)
        st["w_bad"][sl] += done & ~fin
        f = done & fin
        st["w_n"][sl] += f
        err = q0 - g
        for key, v in (("w_q", q0), ("w_g", g), ("w_e", err), ("w_e2", err * err), ("w_q2", q0 * q0), ("w_g2", g * g),
                       ("w_qg", q0 * g)):
            st[key][sl] = np.where(f, st[key][sl] + v, st[key][sl])
        st["w_emin"][sl] = np.where(f & (err < st["w_emin"][sl]), err, st["w_emin"][sl])
        st["w_emax"][sl] = np.where(f & (err > st["w_emax"][sl]), err, st["w_emax"][sl])
        st["open"][sl] = np.where(done, 0, 1)


def probe_rows(st, layout_idx, n_layouts):
    """evx_vprobe_reduce's rows: a list of 12-tuples (probes, bad, open, q, g, e, e2, q2, g2, qg, emin, emax)."""
    E = len(st["open"])
    li = np.zeros(E, np.int64) if layout_idx is None else np.asarray(layout_idx)
    out = []
    for row in range(n_layouts + 1):
        m = np.ones(E, bool) if row == n_layouts else li == row
        sums = [span_sum(st[k], m) for k in ("w_q", "w_g", "w_e", "w_e2", "w_q2", "w_g2", "w_qg")]
        out.append((int(st["w_n"][m].sum()), int(st["w_bad"][m].sum()), int((st["open"][m] != 0).sum()), *sums,
                    float(st["w_emin"][m].min()) if m.any() else np.inf,
                    float(st["w_emax"][m].max()) if m.any() else -np.inf))
    return out


def bits(x):
    """float64 values as their bit patterns (NaN-safe equality, -0.0 != 0.0)."""
    return np.asarray(x, np.float64).reshape(-1).view(np.int64)
