"""The soft decoders' entry points of the C ABI, held to what they answered before their shared
call path (SoftCall, the families, the two drivers of csrc/capi.cpp) replaced ten hand-written ones.

* Error contract: for each of the nine device entries -- the four decodes (flooding, layered,
  fixed-point layered, ensemble) and the five fused Monte-Carlo batches -- and for the host-pointer
  ldpc_bp_decode_batch, a table of bad and edge calls with the return code and a piece of
  ldpc_last_error() that csrc/capi.cpp gave at the parent commit.  The rows are written from that
  file's checks in their order, so a row with two faults names the one that is met first.  Every
  refused call is refused on the host; the rows that are answered LDPC_OK with B > 0 run a
  B = 8, n = 96 batch.  (ldpc_bp_decode_batch does not look at max_iters, so it has no such row.)
* Output golden (tests/golden/soft_entries_parent.json, recorded at the parent commit by
  tests/golden/make_soft_entries.py): B = 8, max_iters = 5, one seed, BSC p = 0.07 and AWGN
  sigma = 0.8 (the erasure forms: epsilon = 0.4) -- the whole counter vector of every Monte-Carlo
  entry, and of every decode entry on ldpc_channel_dev's LLRs `its`, a SHA-256 of `hard` and, for
  min-sum (bit-exact by design), of `post`.  Sum-product posteriors: tests/test_gpu_parity.py.
"""
import ctypes as ct
import hashlib
import json
import os

import numpy as np
import pytest

from tests.graph_util import csr_from_checks, regular_simple

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "soft_entries_parent.json")
OK, EINVAL, EHIP, EUNSUP = 0, -1, -3, -5
BEC, BSC, AWGN = 0, 1, 2
N, DV, DC = 96, 3, 6
B, ITERS, SEED = 8, 5, 20261020
PARAM = {BEC: 0.4, BSC: 0.07, AWGN: 0.8}
ALPHA = 0.75

# Parameter names of each entry, in the C ABI's order
DECODE = ("llr", "B", "iters", "algo", "alpha", "early_stop", "post", "hard", "its", "stream")
MC_TAIL = ("expurgation", "stop", "counters", "stream")
ENTRIES = {
    "ldpc_bp_decode_batch_dev": ("g",) + DECODE,
    "ldpc_bp_layered_decode_batch_dev": ("g",) + DECODE,
    "ldpc_bp_layered_q_decode_batch_dev": ("g", "llr", "B", "iters", "q", "early_stop", "post8", "hard", "its", "stream"),
    "ldpc_bp_ensemble_decode_dev": ("n", "dv", "dc", "chk", "var") + DECODE,
    "ldpc_bp_decode_batch": ("v2c", "c2v", "n", "k", "dv", "dc", "h_llr", "B", "iters", "algo", "alpha", "early_stop",
                             "h_post", "h_hard", "h_its"),
    "ldpc_mc_batch_dev": ("g", "channel", "param", "seed", "first_cw", "B", "iters", "algo", "alpha", "early_stop")
    + MC_TAIL,
    "ldpc_mc_layered_batch_dev": ("g", "channel", "param", "seed", "first_cw", "B", "iters", "algo", "alpha",
                                  "early_stop") + MC_TAIL,
    "ldpc_mc_layered_q_batch_dev": ("g", "channel", "param", "seed", "first_cw", "B", "iters", "q", "early_stop")
    + MC_TAIL,
    "ldpc_mc_ensemble_batch_dev": ("n", "dv", "dc", "channel", "param", "seed", "first_cw", "B", "iters") + MC_TAIL,
    "ldpc_mc_ensemble_soft_batch_dev": ("n", "dv", "dc", "channel", "param", "algo", "alpha", "early_stop", "seed",
                                        "first_cw", "B", "iters") + MC_TAIL,
}


class Ref:
    """A value of the environment, named in the table before the environment exists"""

    def __init__(self, name):
        self.name = name


TWICE, DEG36, BAD_Q = Ref("g_twice"), Ref("g_deg36"), Ref("q_bad")
CHANNEL = {"channel": BSC, "param": PARAM[BSC]}
BEC_CH = {"channel": BEC, "param": PARAM[BEC]}
SOFT_ARGS, MC_ARGS, ENS_ARGS = "bad soft batch arguments", "bad MC arguments", "bad ensemble soft batch arguments"
ALGO, CONSISTENT = "algo must be LDPC_ALGO_SPA or LDPC_ALGO_MINSUM", "consistent edge lists"
NO_SCHEDULE, LAYERED_BEC = "graph has no layer schedule", "the layered schedule decodes the BSC and the BI-AWGN"
SHAPE = "need n*dv divisible by dc"

# entry -> rows of (what differs from a good call, return code, piece of the error text)
TABLE = {
    "ldpc_bp_decode_batch_dev": [
        ({}, OK, None),
        ({"B": 0, "llr": None}, OK, None),
        ({"g": None}, EINVAL, SOFT_ARGS),
        ({"llr": None}, EINVAL, SOFT_ARGS),
        ({"B": -1}, EINVAL, SOFT_ARGS),
        ({"iters": -1}, EINVAL, SOFT_ARGS),
        ({"algo": 2}, EINVAL, ALGO),
        ({"algo": -1, "B": 0}, EINVAL, ALGO),
        ({"iters": -1, "algo": 2}, EINVAL, SOFT_ARGS),
        ({"g": DEG36}, EUNSUP, "no soft kernel for this graph (check degree > 32)"),
        ({"g": DEG36, "B": 0}, EUNSUP, "no soft kernel for this graph"),
        ({"g": DEG36, "algo": 2}, EINVAL, ALGO),
    ],
    "ldpc_bp_decode_batch": [
        ({}, OK, None),
        ({"B": 0, "h_llr": None}, OK, None),
        ({"h_llr": None}, EINVAL, SOFT_ARGS),
        ({"B": -1}, EINVAL, SOFT_ARGS),
        ({"algo": 2}, EINVAL, ALGO),
        ({"algo": 2, "v2c": None}, EINVAL, ALGO),
        ({"v2c": None}, EINVAL, "null edge list"),
        ({"c2v": None, "B": 0}, EINVAL, "null edge list"),
        ({"k": N}, EINVAL, "bad (n, k, dv, dc)"),
        # the same graph as the _dev form's LDPC_EUNSUP rows: here the launcher refuses it
        ({"v2c": Ref("deg36_v2c"), "c2v": Ref("deg36_c2v"), "n": 72, "k": 66, "dv": 3, "dc": 36}, EHIP,
         "invalid argument"),
    ],
    "ldpc_bp_layered_decode_batch_dev": [
        ({}, OK, None),
        ({"B": 0, "llr": None}, OK, None),
        ({"g": None}, EINVAL, SOFT_ARGS),
        ({"llr": None}, EINVAL, SOFT_ARGS),
        ({"B": -1}, EINVAL, SOFT_ARGS),
        ({"iters": -1}, EINVAL, SOFT_ARGS),
        ({"algo": 2}, EINVAL, ALGO),
        ({"g": TWICE}, EUNSUP, NO_SCHEDULE),
        ({"g": TWICE, "B": 0}, EUNSUP, NO_SCHEDULE),
        ({"g": TWICE, "algo": 2}, EINVAL, ALGO),
        ({"g": DEG36}, EUNSUP, NO_SCHEDULE),
    ],
    "ldpc_bp_layered_q_decode_batch_dev": [
        ({}, OK, None),
        ({"B": 0, "llr": None}, OK, None),
        ({"g": None}, EINVAL, SOFT_ARGS),
        ({"llr": None}, EINVAL, SOFT_ARGS),
        ({"B": -1}, EINVAL, SOFT_ARGS),
        ({"iters": -1}, EINVAL, SOFT_ARGS),
        ({"q": None}, EINVAL, "null ldpc_quant"),
        ({"q": BAD_Q}, EINVAL, "ldpc_quant: need 2 <= msg_bits <= 7"),
        ({"q": BAD_Q, "B": 0}, EINVAL, "ldpc_quant: need 2 <= msg_bits <= 7"),
        ({"q": None, "g": TWICE}, EINVAL, "null ldpc_quant"),
        ({"g": TWICE}, EUNSUP, NO_SCHEDULE),
        ({"g": DEG36}, EUNSUP, NO_SCHEDULE),
    ],
    "ldpc_bp_ensemble_decode_dev": [
        ({}, OK, None),
        ({"B": 0, "llr": None, "chk": None, "var": None}, OK, None),
        ({"chk": None}, EINVAL, ENS_ARGS),
        ({"var": None}, EINVAL, ENS_ARGS),
        ({"llr": None}, EINVAL, ENS_ARGS),
        ({"B": -1}, EINVAL, ENS_ARGS),
        ({"iters": -1}, EINVAL, ENS_ARGS),
        ({"iters": -1, "n": 97}, EINVAL, ENS_ARGS),
        ({"n": 97}, EINVAL, SHAPE),
        ({"n": 97, "algo": 2}, EINVAL, SHAPE),
        ({"algo": 2}, EINVAL, ALGO),
        ({"n": 72, "dc": 36}, EUNSUP, "no ensemble soft kernel for this shape (check degree > 32)"),
        ({"n": 72, "dc": 36, "B": 0}, EUNSUP, "no ensemble soft kernel for this shape"),
    ],
    "ldpc_mc_batch_dev": [
        (CHANNEL, OK, None),
        (BEC_CH, OK, None),
        (dict(BEC_CH, algo=7), OK, None),  # the erasure decoder has no algo
        (dict(CHANNEL, B=0), OK, None),
        (dict(CHANNEL, g=None), EINVAL, MC_ARGS),
        (dict(CHANNEL, counters=None), EINVAL, MC_ARGS),
        (dict(CHANNEL, B=-1), EINVAL, MC_ARGS),
        (dict(CHANNEL, iters=-1), EINVAL, MC_ARGS),
        ({"channel": 3, "param": 0.1}, EINVAL, "channel must be LDPC_CH_BEC, LDPC_CH_BSC or LDPC_CH_AWGN"),
        ({"channel": 3, "param": 0.1, "algo": 2}, EINVAL, "channel must be"),
        ({"channel": BSC, "param": 0.5}, EINVAL, "BSC crossover probability must be in (0, 0.5)"),
        ({"channel": AWGN, "param": 0.0}, EINVAL, "AWGN sigma must be > 0"),
        ({"channel": BEC, "param": 1.5}, EINVAL, "erasure probability must be in [0, 1]"),
        (dict(CHANNEL, algo=2), EINVAL, "bad algo"),
        (dict(CHANNEL, algo=2, B=0), EINVAL, "bad algo"),
        (dict(CHANNEL, g=DEG36), EHIP, "invalid argument"),  # no up-front check here: the launcher refuses it
        (dict(CHANNEL, g=DEG36, B=0), OK, None),
    ],
    "ldpc_mc_layered_batch_dev": [
        (CHANNEL, OK, None),
        (dict(CHANNEL, B=0), OK, None),
        (dict(CHANNEL, g=None), EINVAL, MC_ARGS),
        (dict(CHANNEL, counters=None), EINVAL, MC_ARGS),
        (dict(CHANNEL, B=-1), EINVAL, MC_ARGS),
        (dict(CHANNEL, iters=-1), EINVAL, MC_ARGS),
        (BEC_CH, EINVAL, LAYERED_BEC),
        (dict(BEC_CH, algo=2), EINVAL, LAYERED_BEC),  # the BEC is rejected before algo is looked at
        ({"channel": BEC, "param": 1.5}, EINVAL, LAYERED_BEC),
        (dict(BEC_CH, g=TWICE), EINVAL, LAYERED_BEC),
        ({"channel": BSC, "param": -0.1}, EINVAL, "BSC crossover probability"),
        ({"channel": BSC, "param": -0.1, "algo": 2}, EINVAL, "BSC crossover probability"),
        ({"channel": AWGN, "param": -1.0}, EINVAL, "AWGN sigma must be > 0"),
        (dict(CHANNEL, algo=2), EINVAL, ALGO),
        (dict(CHANNEL, algo=2, g=TWICE), EINVAL, ALGO),
        (dict(CHANNEL, g=TWICE), EUNSUP, NO_SCHEDULE),
        (dict(CHANNEL, g=TWICE, B=0), EUNSUP, NO_SCHEDULE),
        (dict(CHANNEL, g=DEG36), EUNSUP, NO_SCHEDULE),
    ],
    "ldpc_mc_layered_q_batch_dev": [
        (CHANNEL, OK, None),
        (dict(CHANNEL, B=0), OK, None),
        (dict(CHANNEL, g=None), EINVAL, MC_ARGS),
        (dict(CHANNEL, counters=None), EINVAL, MC_ARGS),
        (dict(CHANNEL, B=-1), EINVAL, MC_ARGS),
        (dict(CHANNEL, iters=-1), EINVAL, MC_ARGS),
        (BEC_CH, EINVAL, LAYERED_BEC),
        (dict(BEC_CH, q=None), EINVAL, LAYERED_BEC),
        ({"channel": BSC, "param": 0.7}, EINVAL, "BSC crossover probability"),
        ({"channel": BSC, "param": 0.7, "q": None}, EINVAL, "BSC crossover probability"),
        (dict(CHANNEL, q=None), EINVAL, "null ldpc_quant"),
        (dict(CHANNEL, q=BAD_Q), EINVAL, "ldpc_quant: need 2 <= msg_bits <= 7"),
        (dict(CHANNEL, q=BAD_Q, g=TWICE), EINVAL, "ldpc_quant: need 2 <= msg_bits <= 7"),
        (dict(CHANNEL, g=TWICE), EUNSUP, NO_SCHEDULE),
        (dict(CHANNEL, g=DEG36, B=0), EUNSUP, NO_SCHEDULE),
    ],
    "ldpc_mc_ensemble_batch_dev": [
        (BEC_CH, OK, None),
        (dict(BEC_CH, B=0), OK, None),
        (dict(BEC_CH, n=97), EINVAL, SHAPE),
        (dict(CHANNEL, n=97), EINVAL, SHAPE),
        (dict(BEC_CH, n=97, counters=None), EINVAL, SHAPE),
        (CHANNEL, EINVAL, "ensemble Monte-Carlo is BEC-only"),
        (dict(CHANNEL, counters=None), EINVAL, "ensemble Monte-Carlo is BEC-only"),
        (dict(BEC_CH, counters=None), EINVAL, MC_ARGS),
        (dict(BEC_CH, B=-1), EINVAL, MC_ARGS),
        (dict(BEC_CH, iters=-1), EINVAL, MC_ARGS),
        ({"channel": BEC, "param": -0.5}, EINVAL, "erasure probability must be in [0, 1]"),
        ({"channel": BEC, "param": -0.5, "iters": -1}, EINVAL, MC_ARGS),
    ],
    "ldpc_mc_ensemble_soft_batch_dev": [
        (CHANNEL, OK, None),
        (dict(CHANNEL, B=0), OK, None),
        (BEC_CH, OK, None),
        (dict(BEC_CH, algo=2), OK, None),  # the BEC is forwarded before any other check
        (dict(BEC_CH, algo=2, n=97), EINVAL, SHAPE),
        (dict(BEC_CH, counters=None), EINVAL, MC_ARGS),
        (dict(CHANNEL, counters=None), EINVAL, MC_ARGS),
        (dict(CHANNEL, counters=None, n=97), EINVAL, MC_ARGS),
        (dict(CHANNEL, B=-1), EINVAL, MC_ARGS),
        (dict(CHANNEL, iters=-1), EINVAL, MC_ARGS),
        ({"channel": 3, "param": 0.1}, EINVAL, "channel must be"),
        ({"channel": BSC, "param": 0.5, "n": 97}, EINVAL, "BSC crossover probability"),
        ({"channel": AWGN, "param": 0.0}, EINVAL, "AWGN sigma must be > 0"),
        (dict(CHANNEL, n=97), EINVAL, SHAPE),
        (dict(CHANNEL, n=97, algo=2), EINVAL, SHAPE),
        (dict(CHANNEL, algo=2), EINVAL, ALGO),
        (dict(CHANNEL, algo=2, n=72, dc=36), EINVAL, ALGO),
        (dict(CHANNEL, n=72, dc=36), EUNSUP, "no ensemble soft kernel for this shape (check degree > 32)"),
        (dict(CHANNEL, n=72, dc=36, B=0), EUNSUP, "no ensemble soft kernel for this shape"),
    ],
}


class Env:
    """Graphs, device and host buffers of every call, and the good call of each entry"""

    def __init__(self):
        import torch
        from iib_project_ldpc_codes_amd import _native
        from iib_project_ldpc_codes_amd.graph import TannerGraph
        assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
        self.torch, self.native, self.lib = torch, _native, _native.lib()
        self.reg = TannerGraph.random_regular(N, DV, DC, seed=7)
        # check 0 holds variable 0 twice: consistent lists, a flooding kernel, no layer schedule
        rows = [[0, 0, 1], [1, 2, 3], [2, 3, 0]]
        self.twice = TannerGraph.from_csr(*csr_from_checks(np.cumsum([0] + [len(r) for r in rows]), np.concatenate(rows), 4))
        self.deg36 = regular_simple(72, 3, 36, seed=1)  # check degree > 32: no soft kernel
        self.quant, self.bad_quant = _native.Quant(2.0, 6, 8, 6, 0), _native.Quant(2.0, 1, 8, 6, 0)

        def dev(shape, dtype):
            return torch.zeros(shape, dtype=dtype, device="cuda")

        self.llr, self.post, self.post8 = dev((B, N), torch.float32), dev((B, N), torch.float32), dev((B, N), torch.int8)
        self.hard, self.its = dev((B, N), torch.uint8), dev(B, torch.int32)
        self.counters = dev(_native.MC_NCOUNT + ITERS + 1, torch.int64)
        self.chk, self.var = dev((B, N * DV), torch.int32), dev((B, N * DV), torch.int32)
        rc = self.lib.ldpc_sample_regular_dev(N, DV, DC, SEED, 0, B, self.chk.data_ptr(), self.var.data_ptr(), None, None)
        assert rc == 0, _native.last_error()
        self.h_llr, self.h_post = np.zeros((B, N), np.float32), np.zeros((B, N), np.float32)
        self.h_hard, self.h_its = np.zeros((B, N), np.uint8), np.zeros(B, np.int32)
        self.lists = {g: (np.ascontiguousarray(g.variable_lookup, np.int32), np.ascontiguousarray(g.check_lookup, np.int32))
                      for g in (self.reg, self.deg36)}
        v2c, c2v = self.lists[self.reg]
        self.values = {
            "g": self.reg.handle(), "g_twice": self.twice.handle(), "g_deg36": self.deg36.handle(),
            "q": ct.addressof(self.quant), "q_bad": ct.addressof(self.bad_quant),
            "llr": self.llr.data_ptr(), "post": self.post.data_ptr(), "post8": self.post8.data_ptr(),
            "hard": self.hard.data_ptr(), "its": self.its.data_ptr(), "counters": self.counters.data_ptr(),
            "chk": self.chk.data_ptr(), "var": self.var.data_ptr(), "stream": None,
            "h_llr": self.h_llr.ctypes.data, "h_post": self.h_post.ctypes.data, "h_hard": self.h_hard.ctypes.data,
            "h_its": self.h_its.ctypes.data, "v2c": v2c.ctypes.data, "c2v": c2v.ctypes.data,
            "deg36_v2c": self.lists[self.deg36][0].ctypes.data, "deg36_c2v": self.lists[self.deg36][1].ctypes.data,
            "n": N, "k": self.reg.k, "dv": DV, "dc": DC, "B": B, "iters": ITERS, "algo": 1, "alpha": ALPHA,
            "early_stop": 0, "seed": SEED, "first_cw": 0, "expurgation": -1, "stop": 0,
        }

    def call(self, entry, **change):
        """The entry's good call with `change` applied; (return code, ldpc_last_error())"""
        args = []
        for name in ENTRIES[entry]:
            v = change[name] if name in change else self.values[name]
            args.append(self.values[v.name] if isinstance(v, Ref) else v)
        unknown = set(change) - set(ENTRIES[entry])
        assert not unknown, (entry, unknown)
        rc = getattr(self.lib, entry)(*args)
        return rc, self.native.last_error()

    def channel(self, kind):
        rc = self.lib.ldpc_channel_dev(kind, PARAM[kind], SEED, 0, N, B, self.llr.data_ptr(), None)
        assert rc == 0, self.native.last_error()
        self.torch.cuda.synchronize()
        self.h_llr[:] = self.llr.cpu().numpy()


@pytest.fixture(scope="module")
def env():
    return Env()


@pytest.mark.parametrize("entry", sorted(TABLE))
def test_error_contract(env, entry):
    wrong = []
    for change, code, text in TABLE[entry]:
        rc, err = env.call(entry, **change)
        shown = {k: (v.name if isinstance(v, Ref) else v) for k, v in change.items()}
        print(entry, shown, "->", rc, repr(err) if rc else "")
        if rc != code or (text is not None and text not in err):
            wrong.append((shown, "expected", code, text, "got", rc, err))
    env.torch.cuda.synchronize()
    assert all(text is not None for _, code, text in TABLE[entry] if code != OK)  # every refusal names its text
    assert not wrong, wrong


def _sha(t):
    return hashlib.sha256(np.ascontiguousarray(t.cpu().numpy()).tobytes()).hexdigest()


def record(env):
    """What the golden holds: name of the call -> counters, or {its, hard[, post]}"""
    out = {}
    modes = [(algo, es) for algo in (0, 1) for es in (0, 1)]

    def mc(entry, kind, tag, **change):
        env.counters.zero_()
        rc, err = env.call(entry, channel=kind, param=PARAM[kind], **change)
        assert rc == 0, (entry, tag, err)
        env.torch.cuda.synchronize()
        out["%s/%s" % (entry, tag)] = [int(x) for x in env.counters.cpu().numpy()]

    mc("ldpc_mc_batch_dev", BEC, "bec")
    mc("ldpc_mc_ensemble_batch_dev", BEC, "bec")
    mc("ldpc_mc_ensemble_soft_batch_dev", BEC, "bec")
    for kind, ch in ((BSC, "bsc"), (AWGN, "awgn")):
        for algo, es in modes:
            tag = "%s/algo%d/es%d" % (ch, algo, es)
            for entry in ("ldpc_mc_batch_dev", "ldpc_mc_layered_batch_dev", "ldpc_mc_ensemble_soft_batch_dev"):
                mc(entry, kind, tag, algo=algo, early_stop=es)
        for es in (0, 1):
            mc("ldpc_mc_layered_q_batch_dev", kind, "%s/es%d" % (ch, es), early_stop=es)

    def decode(entry, tag, minsum, post, **change):
        for t in (env.post, env.post8, env.hard, env.its):
            t.zero_()
        rc, err = env.call(entry, **change)
        assert rc == 0, (entry, tag, err)
        env.torch.cuda.synchronize()
        got = {"its": [int(x) for x in env.its.cpu().numpy()], "hard": _sha(env.hard)}
        if minsum:
            got["post"] = _sha(post)
        out["%s/%s" % (entry, tag)] = got

    for kind, ch in ((BSC, "bsc"), (AWGN, "awgn")):
        env.channel(kind)
        for algo, es in modes:
            tag = "%s/algo%d/es%d" % (ch, algo, es)
            for entry in ("ldpc_bp_decode_batch_dev", "ldpc_bp_layered_decode_batch_dev", "ldpc_bp_ensemble_decode_dev"):
                decode(entry, tag, algo == 1, env.post, algo=algo, early_stop=es)
            rc, err = env.call("ldpc_bp_decode_batch", algo=algo, early_stop=es)
            assert rc == 0, err
            got = {"its": [int(x) for x in env.h_its], "hard": hashlib.sha256(env.h_hard.tobytes()).hexdigest()}
            if algo == 1:
                got["post"] = hashlib.sha256(env.h_post.tobytes()).hexdigest()
            out["ldpc_bp_decode_batch/" + tag] = got
        for es in (0, 1):
            decode("ldpc_bp_layered_q_decode_batch_dev", "%s/es%d" % (ch, es), True, env.post8, early_stop=es)
    return out


def test_outputs_match_parent_golden(env):
    with open(GOLDEN) as f:
        golden = json.load(f)
    got = record(env)
    assert golden["inputs"] == {"n": N, "dv": DV, "dc": DC, "B": B, "max_iters": ITERS, "seed": SEED, "alpha": ALPHA,
                                "bec": PARAM[BEC], "bsc": PARAM[BSC], "awgn": PARAM[AWGN]}
    assert sorted(got) == sorted(golden["calls"])
    wrong = {k: (got[k], golden["calls"][k]) for k in got if got[k] != golden["calls"][k]}
    assert not wrong, wrong
