"""The shape tables (csrc/kernel_shapes.hpp) through the shape-only plan entries, no device needed:
over sweeps of sizes across every threshold of the BEC, Gallager A/B, encoder and sampler plans,
the display name of each plan row is exactly the string formed from the row's own columns
(threads, plane words, plane bytes, modes, tile width, ring and row widths), and a row is named
"none" exactly when it has no kernel.  The launchers pick the instantiation by the same columns, so
a name that disagreed with them would name a kernel that does not run."""
from tests import encode_util, gallager_util, sampler_shapes_util as shapes
from tests.graph_util import BEC_DECODE, BEC_MC, bec_plans

# 64 .. 200,000 in steps of 3 %, and both sides of every power of two and of the plans' thresholds
SIZES = sorted({int(64 * 1.03 ** k) for k in range(273)} | {200000} |
               {x + d for x in (2048, 4096, 8192, 16384, 32768, 65536, 131072) for d in (-1, 0, 1)})
assert SIZES[0] == 64 and SIZES[-1] == 200000 and len(SIZES) > 250


BEC_ROWS = {"bec_%s_bits_kernel<%s>" % (kind, row) for kind in ("dec", "mc")
            for row in ("1024,1,u8", "256,4,u32", "256,2,u32", "256,1,u32", "512,4,u32", "512,2,u32", "512,1,u32")}
BEC_ROWS |= {"bec_kernel<1024>", "bec_kernel<256>", "none"}


def test_bec_names_are_their_rows():
    kernels = set()
    # (2^17 trials: the smallest power of two at which Monte-Carlo takes four plane words)
    calls = [(mode, B, 50) for mode in (BEC_DECODE, BEC_MC) for B in (1, 63, 64, 4096, 65536, 1 << 17)]
    # rate 1/2, and few checks (where 512 threads still take four plane words)
    for n, m in [(n, n // 2) for n in SIZES] + [(n, n // 16) for n in SIZES[::4]]:
        for (mode, _, _), p in zip(calls, bec_plans(n, m, calls)):
            if p["kernel"] in ("DecBits", "McBits"):
                assert p["kernel"] == ("DecBits" if mode == BEC_DECODE else "McBits")
                want = "bec_%s_bits_kernel<%d,%d,u%d>" % ("dec" if mode == BEC_DECODE else "mc", p["threads"], p["W"],
                                                         8 * p["plane"])
            elif p["kernel"] == "Word":
                want = "bec_kernel<%d>" % p["threads"]
            else:
                assert p["kernel"] == "None" and p["threads"] == 0
                want = "none"
            assert p["name"] == want, (n, p)
            assert (p["name"] == "none") == (p["kernel"] == "None") == (p["threads"] == 0), (n, p)
            kernels.add(p["name"])
    # the sweep reaches every row of both modes, both word rows and the call that nothing holds
    assert kernels == BEC_ROWS, sorted(kernels ^ BEC_ROWS)


def test_gb_names_are_their_rows():
    kernels = set()
    modes = [(es, mc) for es in (0, 1) for mc in (0, 1)]
    for n in SIZES:
        for E in (3 * n, 15 * n):
            for (es, mc), p in zip(modes, gallager_util.gb_plans(n, E, [(33, 20, es, mc) for es, mc in modes])):
                want = "none"
                if p["threads"]:
                    want = "gb_kernel<%d,u%d%s%s>" % (p["threads"], 8 * p["plane"], ",es" if es else "", ",mc" if mc else "")
                assert p["name"] == want, (n, E, p)
                assert (p["name"] == "none") == (p["threads"] == 0) == (p["plane"] == 0), (n, E, p)
                kernels.add(p["name"])
    assert len(kernels) == 4 * 4 + 1, sorted(kernels)


def test_encode_names_are_their_rows():
    ks = sorted({0, 1, 60000} | {int(1.03 ** k) for k in range(373)} |
                {x + d for x in (9984, 19968, 20480, 39936) for d in (-1, 0, 1)})
    assert ks[-1] == 60000
    rc, rows = encode_util.encode_plans([(K + 7, K, 7, 33) for K in ks])
    assert rc != 0  # some K has no tile (its row: "none")
    names = set()
    for K, p in zip(ks, rows):
        want = "encode_parity_kernel<%d>" % p["W"] if p["threads"] else "none"
        assert p["name"] == want, (K, p)
        assert (p["name"] == "none") == (p["threads"] == 0) == (p["W"] == 0), (K, p)
        names.add(p["name"])
    assert names == {"none", "encode_parity_kernel<1>", "encode_parity_kernel<2>", "encode_parity_kernel<4>"}


def test_sampler_names_are_their_rows():
    names = set()
    for args, p in shapes.sweep_plans():
        form = "regular" if args[5] else "csr"
        if p["seq"]:
            assert p["K"] == 0 and p["ring"] in (2, 4)
            draw = "sample_seq_kernel<%s,%s>" % (form, "u16" if p["ring"] == 2 else "int")
        else:
            assert p["K"] in (256, 512, 1024)
            draw = "sample_regular_kernel<%d,%s>" % (p["K"], "int32,gmem" if p["K"] == 1024 else "u16,lds")
        search = "none"
        if p["W"]:
            assert p["seq"]
            search = "sample_search_kernel<%s,%s>" % (form, "u16" if p["ring"] == 2 else "int")
        var_side = "none"
        if p["V"]:
            assert p["seq"] and p["row"] in (2, 4)
            var_side = "sample_var_side_kernel<1024,%s>" % ("u16" if p["row"] == 2 else "int32")
        assert (p["draw"], p["search"], p["var_side"]) == (draw, search, var_side), (args, p)
        assert p["threads"] > 0 and p["draw"] != "none", (args, p)  # every shape of the sweep has a draw kernel
        names |= {draw, search, var_side}
    assert len(names) == 3 + 4 + 4 + 2 + 1, sorted(names)
