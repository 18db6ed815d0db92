"""The fp64 twin of the field-aware FM (include/fmhip_ffm.h), straight from the header's formulas: loops over pairs, nothing clever.
Rows are lists of (field, feature, value).  A plain FM is the same model with every field id 0 (F = 1)."""
import numpy as np


class State:
    def __init__(self, w0, w, v, init=None):
        self.w0, self.w, self.v = float(w0), np.array(w, np.float64), np.array(v, np.float64)
        if init is not None:          # AdaGrad's accumulators
            self.n0, self.nw, self.nv = float(init), np.full_like(self.w, init), np.full_like(self.v, init)


def predict_row(s, row):
    """(yhat, sum of |terms|) of one row."""
    yh, mag = s.w0, abs(s.w0)
    for f, i, x in row:
        yh += s.w[i] * x
        mag += abs(s.w[i] * x)
    for a in range(len(row)):
        for b in range(a + 1, len(row)):
            (fa, ia, xa), (fb, ib, xb) = row[a], row[b]
            t = xa * xb * float(s.v[ia, fb] @ s.v[ib, fa])
            yh += t
            mag += abs(t)
    return yh, mag


def predict(s, rows):
    out = np.array([predict_row(s, r) for r in rows], np.float64).reshape(-1, 2)
    return out[:, 0], out[:, 1]


def logloss(s, rows, y):
    yh = predict(s, rows)[0]
    return float(np.mean(np.maximum(yh, 0.0) - (y > 0) * yh + np.log1p(np.exp(-np.abs(yh)))))


def step(s, rows, y, eta, reg0, regw, regv, loss="squared", optimizer="sgd", eps=1e-10, linear=True):
    """One mini-batch step in place -> (touched_v [n + 1, F] bool, touched_w [n + 1] bool)."""
    B = len(rows)
    yh, y = predict(s, rows)[0], np.asarray(y, np.float64)
    e = yh - y if loss == "squared" else 1.0 / (1.0 + np.exp(-yh)) - (y > 0)
    gv, gw = np.zeros_like(s.v), np.zeros_like(s.w)
    tv, tw = np.zeros(s.v.shape[:2], bool), np.zeros(s.w.shape, bool)
    for r, row in enumerate(rows):
        for a, (fa, ia, xa) in enumerate(row):
            gw[ia] += e[r] * xa / B
            tw[ia] = True
            for b, (fb, ib, xb) in enumerate(row):
                if b != a:
                    gv[ia, fb] += e[r] * xa * xb * s.v[ib, fa] / B
                    tv[ia, fb] = True
    g0 = e.sum() / B

    def upd(theta, n, g, mask):
        if optimizer == "sgd":
            return np.where(mask, theta - eta * g, theta), n
        n2 = n + g * g
        return np.where(mask, theta - eta * g / (np.sqrt(n2) + eps), theta), np.where(mask, n2, n)

    nv, nw, n0 = (s.nv, s.nw, s.n0) if optimizer == "adagrad" else (None, None, None)
    s.v, nv = upd(s.v, nv, gv + regv * s.v, tv[:, :, None])
    if linear:
        s.w, nw = upd(s.w, nw, gw + regw * s.w, tw)
        w0, n0 = upd(s.w0, n0, g0 + reg0 * s.w0, True)
        s.w0 = float(w0)
    else:
        tw[:] = False
    if optimizer == "adagrad":
        s.nv, s.nw, s.n0 = nv, nw, float(n0)
    return tv, tw


def epoch(s, rows, y, batch_rows, order=None, **kw):
    n = len(rows)
    br = n if batch_rows <= 0 else batch_rows
    starts = list(range(0, n, br))
    for j in (range(len(starts)) if order is None else order):
        lo = starts[j]
        step(s, rows[lo:lo + br], y[lo:lo + br], **kw)
    return s


def layout(rows, batch_rows, chunk):
    """The dataset build's layout as the harness prints it: per row its entries sorted by (field, feature) with the run heads' lengths
    ("row r: f:i:run ..."), per batch its columns with their occurrences (row, position) and chunk cuts ("batch b col i chunks c: r.p ...")."""
    lines = []
    srt = [sorted(r, key=lambda e: (e[0], e[1])) for r in rows]
    for r, row in enumerate(srt):
        items = []
        for p, (f, i, _) in enumerate(row):
            head = p == 0 or row[p - 1][0] != f
            run = sum(1 for q in row if q[0] == f) if head else 0
            items.append("%d:%d:%d" % (f, i, run))
        lines.append("row %d: %s" % (r, " ".join(items)))
    n = len(rows)
    br = n if batch_rows <= 0 or batch_rows > n else batch_rows
    for b, lo in enumerate(range(0, n, br)):
        occ = {}
        for r in range(lo, min(n, lo + br)):
            for p, (_, i, _) in enumerate(srt[r]):
                occ.setdefault(i, []).append("%d.%d" % (r - lo, p))
        for i in sorted(occ):
            lines.append("batch %d col %d chunks %d: %s" % (b, i, (len(occ[i]) + chunk - 1) // chunk, " ".join(occ[i])))
    return "\n".join(lines) + "\n"


def random_rows(rng, n_rows, n1, F, lengths, one_field_row=True):
    """Rows whose lengths cycle through `lengths` (capped by n1), fields drawn with repeats (runs longer than 1), distinct features
    per row including ids 0 and n1 - 1, one explicit zero value; with one_field_row the last row is a single field."""
    rows = []
    for r in range(n_rows):
        L = min(lengths[r % len(lengths)], n1)
        feats = rng.choice(n1, L, replace=False)
        if L >= 2:
            feats[:2] = [0, n1 - 1] if r % 3 == 0 else feats[:2]
            feats = np.array(list(dict.fromkeys(feats.tolist())))
        fields = rng.integers(0, F, len(feats))
        vals = rng.normal(0, 1, len(feats))
        if len(feats) > 1 and r % 4 == 1:
            vals[1] = 0.0
        rows.append([(int(f), int(i), float(x)) for f, i, x in zip(fields, feats, vals)])
    if one_field_row and rows:
        rows[-1] = [(F - 1, i, x) for _, i, x in rows[-1]]
    return rows


# ---- the planted task: pair weights that depend on the partner's FIELD --------------------------------------------------------
P_FIELDS, P_PER_FIELD, P_K, P_TRAIN, P_TEST, P_BATCH, P_EPOCHS = 3, 20, 4, 600, 600, 5, 20
P_ETA, P_REGV, P_TRUE_RANK, P_TRUE_SCALE = 0.2, 0.01, 2, 2.0


def planted(seed=7):
    """One categorical feature per field (3 entries a row, value 1); the label is a draw from sigma of a true FFM's score whose
    vectors V*[i][f] are independent per field: what feature i means to field 1 says nothing about what it means to field 2.  The
    truth has rank 2 per field pair: an FFM of k = 4 holds it, a plain FM would need 2 factors per field PAIR, 6 > 4."""
    rng = np.random.default_rng(seed)
    n1 = P_FIELDS * P_PER_FIELD
    vt = np.zeros((n1, P_FIELDS, P_K))
    vt[:, :, :P_TRUE_RANK] = rng.normal(0, P_TRUE_SCALE, (n1, P_FIELDS, P_TRUE_RANK))
    truth = State(0.0, np.zeros(n1), vt)

    def draw(n):
        rows = [[(f, f * P_PER_FIELD + int(rng.integers(P_PER_FIELD)), 1.0) for f in range(P_FIELDS)] for _ in range(n)]
        p = 1.0 / (1.0 + np.exp(-predict(truth, rows)[0]))
        return rows, (rng.random(n) < p).astype(np.float64)
    return dict(n1=n1, train=draw(P_TRAIN), test=draw(P_TEST), seed=seed)


def planted_init(t, F):
    v = np.random.default_rng(t["seed"] + 1).random((t["n1"], F, P_K)) / np.sqrt(P_K)       # libffm's init
    return State(0.0, np.zeros(t["n1"]), v, init=1.0)


def run_planted(t, fm=False, epochs=P_EPOCHS):
    """Trains the twin (the plain FM with fm=True) -> (state, train log-loss, test log-loss)."""
    conv = (lambda rows: [[(0, i, x) for _, i, x in r] for r in rows]) if fm else (lambda rows: rows)          # a plain FM: every field 0
    (xtr, ytr), (xte, yte) = t["train"], t["test"]
    xtr, xte = conv(xtr), conv(xte)
    s = planted_init(t, 1 if fm else P_FIELDS)
    for _ in range(epochs):
        epoch(s, xtr, ytr, P_BATCH, eta=P_ETA, reg0=0.0, regw=0.0, regv=P_REGV, loss="logistic", optimizer="adagrad")
    return s, logloss(s, xtr, ytr), logloss(s, xte, yte)
