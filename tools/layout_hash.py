#!/usr/bin/env python3
"""Prints hashes of how fmhip_dataset_create laid fixed, seeded datasets out and of what a model computes over that layout — one
line per case: SHA-256 prefixes of layout() (hot ids, stream sizes, band plan), of every batch's batch_info, of every array of
every batch's transposeInput, the ALS level figures, the bits of predict and of every batch's batchGradient, %.17g of each sse.
Run it with two builds of the library (FMHIP_LIB=sparkfm_amd/lib/libfmhip_<name>.so, tools/build_variant.sh): a change to the
dataset build that moves no entry leaves every line as it was.  The sibling of tools/grad_hash.py and tools/score_hash.py.
    python3 tools/layout_hash.py
Cases: a hot block with refused features at 2 and at 8 pages; a thin first page; every feature hot (and an empty row); a single
batch (the fp64 ALS copies) with and without a feature stored twice in a row; row-blocked transposes; float32 arrays as
scoring-only rows and as a training dataset; k = 64 under FMHIP_ORDER_WINDOW=64; one batch large enough for the band plan."""
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import sparkfm_amd as fmhip  # noqa: E402
from sparkfm_amd import synth  # noqa: E402
from test_gpu_parity import hot_problem  # noqa: E402


def sha(*arrays):
    return hashlib.sha256(b"".join(np.ascontiguousarray(a).tobytes() for a in arrays)).hexdigest()[:12]


def sha_text(obj):
    return hashlib.sha256(repr(obj).encode()).hexdigest()[:12]


def case(tag, a, env=None, **kw):
    """builds the dataset of arrays `a` (keys as hot_problem returns them) with DataSet keywords `kw` and prints its line"""
    for key, value in (env or {}).items():
        os.environ[key] = value
    try:
        ds = fmhip.DataSet(a["row_ptr"], a["col"], a["val"], a["y"], **kw).cache()
    finally:
        for key in env or {}:
            del os.environ[key]
    nb, lay = ds.n_batches, ds.layout()
    out = ["layout %s (%d pages, %d dense ids, %d of %d ranges planned)" % (sha_text(sorted(lay.items())), lay["hot_pages"], len(lay["hot_ids_all"]),
                                                                          lay["planned_ranges"], lay["ranges"]), "batches %d %s" % (nb, sha_text([sorted(ds.batch_info(b).items()) for b in range(nb)])),
           "als %s" % sha_text(sorted(ds.alsLevels().items()))]
    fm = fmhip.FMModel(a["n1"] - 1, a["k"])
    fm.w0, fm.w, fm.v = a["w0"], a["w"], a["v"]
    out.append("predict %s" % sha(fm.predict(ds)))
    if not kw.get("scoring"):
        out.append("transposes %s" % " ".join(sha(*ds.transposeInput(b)) for b in range(nb)))
        grads = []
        for b in range(nb):
            gv, gw, g0, st = fm.batchGradient(ds, b)
            grads.append("%s g0 %.17g sse %.17g" % (sha(gv, gw), g0, st["sse"]))
        out.append("gradients %s" % " ; ".join(grads))
    print("%s: %s" % (tag, " | ".join(out)), flush=True)
    fm.close()
    ds.unpersist()


def zipf_problem(seed, rows, n1, lo, hi, k):
    d = synth.make_zipf(seed, rows, n1, lo, hi, zipf_s=1.05)
    _, _, v = synth.init_params(seed + 4, n1, k, stdev=0.05)
    return dict(k=k, n1=n1, w0=0.1, w=np.random.default_rng(seed).normal(0, 0.05, n1), v=v, row_ptr=d["row_ptr"], col=d["col"], val=d["val"], y=d["y"])


def dense_problem(seed, rows, n1, k, empty_row):
    """every one of the n1 features in 30-90 % of the rows; one row without entries"""
    rng = np.random.default_rng(seed)
    present = rng.random((rows, n1)) < rng.uniform(0.3, 0.9, n1)
    present[empty_row] = False
    _, c = np.nonzero(present)
    row_ptr = np.concatenate([[0], np.cumsum(present.sum(axis=1))]).astype(np.int64)
    return dict(k=k, n1=n1, w0=0.25, w=rng.normal(0, 0.1, n1), v=rng.normal(0, 0.1, (k, n1)), row_ptr=row_ptr, col=c.astype(np.int32),
                val=rng.uniform(0.1, 1.0, len(c)), y=rng.normal(0, 1, rows))


def main():
    a, _ = hot_problem(9101, 3000, 500, 32, 41, 20, 30)
    for pages in (2, 8):
        case("1 refusals, %d pages" % pages, a, batch_rows=700, hot_block=pages)
    a, _ = hot_problem(9102, 4000, 600, 32, 30, n_low=27)
    case("2 thin first page", a, batch_rows=900, hot_block=8)
    case("3 every feature hot", dense_problem(9103, 900, 10, 16, empty_row=450), batch_rows=250)
    for dup in (3, None):
        a, _ = hot_problem(9104, 300, 40, 8, 6, dup)
        case("4 single batch, %s" % ("a feature twice in a row" if dup is not None else "no duplicates"), a)
    a, _ = hot_problem(9105, 1500, 400, 32, 40, 5, 9, 12)
    case("5 row-blocked", a, batch_rows=400, row_block_rows=128)
    a, _ = hot_problem(9106, 2000, 300, 32, 24, 2, 7, 4)
    a.update(val=a["val"].astype(np.float32), y=a["y"].astype(np.float32))
    case("6 float32 scoring rows", a, scoring=True)
    case("6 float32 training", a, batch_rows=600)
    a, _ = hot_problem(9107, 2500, 700, 64, 50, 11, None, 20)
    case("7 k = 64, order window 64", a, env={"FMHIP_ORDER_WINDOW": "64"}, batch_rows=800)
    case("8 one batch, band plan", zipf_problem(9108, 8000, 3000, 8, 16, 32))


if __name__ == "__main__":
    main()
