// Graph preparation: see graph_host.hpp.  Host-only and pure (no HIP call, no getenv).
#include "graph_host.hpp"

#ifndef LDPC_IRR
#define LDPC_IRR 1  // irregular graphs on bp_irr_kernel when in range
#endif
#ifndef LDPC_LOC_LAYOUT
#define LDPC_LOC_LAYOUT 1  // build the local-edge layout (bp_loc_kernel) for rate-1/2 graphs
#endif
#ifndef LDPC_LOC_CHAIN
#define LDPC_LOC_CHAIN 1  // build the chained layout beside it where the shape allows
#endif

namespace ldpc {

// Regular edge lists in the reference format (random_code_generator.c:34-36, :57-62).
int host_graph_from_lists(const int32_t *v2c, const int32_t *c2v, int n, int k, int dv, int dc, HostGraph &h) {
    LDPC_REQUIRE(v2c && c2v, "null edge list");
    LDPC_REQUIRE(n > 0 && dv > 0 && dc > 0 && k >= 0 && k < n, "bad (n, k, dv, dc)");
    const int m = n - k;
    h.n = n; h.m = m; h.k = k; h.dv = dv; h.dc = dc;
    h.max_vdeg = dv; h.max_cdeg = dc;
    const size_t Ec = (size_t)m * dc, Ev = (size_t)n * dv;
    h.cvar.assign(c2v, c2v + Ec);
    for (size_t e = 0; e < Ec; ++e)
        LDPC_REQUIRE(h.cvar[e] >= 0 && h.cvar[e] < n, "check_to_variable_list entry out of range [0, n)");
    for (size_t e = 0; e < Ev; ++e)
        LDPC_REQUIRE(v2c[e] >= 0 && v2c[e] < m, "variable_to_check_list entry out of range [0, n-k)");
    h.cptr.resize(m + 1);
    for (int c = 0; c <= m; ++c) h.cptr[c] = c * dc;
    h.vptr.resize(n + 1);
    for (int v = 0; v <= n; ++v) h.vptr[v] = v * dv;
    h.vchk.resize(Ev);
    h.vslot.assign(Ev, -1);
    bool ok = (Ec == Ev);
    for (int v = 0; v < n; ++v) {
        for (int j = 0; j < dv; ++j) {
            const int c = v2c[(size_t)v * dv + j];
            int occ = 0, rep = 0, found = -1;
            for (int jj = 0; jj < j; ++jj) rep += (v2c[(size_t)v * dv + jj] == c);
            for (int s = 0; s < dc; ++s) {
                if (h.cvar[(size_t)c * dc + s] == v) {
                    if (occ == rep) found = c * dc + s;
                    ++occ;
                }
            }
            h.vchk[(size_t)v * dv + j] = occ == 1 ? c : -1;
            if (found < 0) ok = false;
            h.vslot[(size_t)v * dv + j] = found;
        }
    }
    h.consistent = ok;
    return LDPC_OK;
}

int host_graph_from_csr(const int32_t *cptr, const int32_t *cvar, const int32_t *vptr, const int32_t *vslot, int n,
                        int m, HostGraph &h) {
    LDPC_REQUIRE(cptr && cvar && vptr && vslot && n > 0 && m > 0, "bad CSR graph arguments");
    LDPC_REQUIRE(cptr[0] == 0 && vptr[0] == 0 && cptr[m] == vptr[n] && cptr[m] > 0, "CSR pointers disagree");
    const int E = cptr[m];
    h.n = n; h.m = m; h.k = n - m;
    h.cptr.assign(cptr, cptr + m + 1);
    h.vptr.assign(vptr, vptr + n + 1);
    h.cvar.assign(cvar, cvar + E);
    h.vslot.assign(vslot, vslot + E);
    std::vector<int32_t> slot_check(E);
    for (int c = 0; c < m; ++c) {
        LDPC_REQUIRE(cptr[c + 1] >= cptr[c], "check_ptr not monotone");
        h.max_cdeg = std::max(h.max_cdeg, cptr[c + 1] - cptr[c]);
        for (int s = cptr[c]; s < cptr[c + 1]; ++s) {
            LDPC_REQUIRE(cvar[s] >= 0 && cvar[s] < n, "check_var out of range");
            slot_check[s] = c;
        }
    }
    std::vector<char> seen(E, 0);
    h.vchk.resize(E);
    for (int v = 0; v < n; ++v) {
        LDPC_REQUIRE(vptr[v + 1] >= vptr[v], "var_ptr not monotone");
        h.max_vdeg = std::max(h.max_vdeg, vptr[v + 1] - vptr[v]);
        for (int e = vptr[v]; e < vptr[v + 1]; ++e) {
            const int s = vslot[e];
            LDPC_REQUIRE(s >= 0 && s < E && !seen[s] && cvar[s] == v, "var_slot is not a slot permutation");
            seen[s] = 1;
            const int c = slot_check[s];
            int occ = 0;
            for (int q = cptr[c]; q < cptr[c + 1]; ++q) occ += (cvar[q] == v);
            h.vchk[e] = occ == 1 ? c : -1;
        }
    }
    bool reg_c = true, reg_v = true;
    for (int c = 0; c < m; ++c) reg_c &= (cptr[c + 1] - cptr[c] == h.max_cdeg);
    for (int v = 0; v < n; ++v) reg_v &= (vptr[v + 1] - vptr[v] == h.max_vdeg);
    if (reg_c && reg_v) {
        h.dc = h.max_cdeg;
        h.dv = h.max_vdeg;
    }
    h.consistent = true;
    return LDPC_OK;
}

// Conflict-aware lane layout for the LDS-resident kernel (bp_lds_kernel).
// Lane positions p = t + i*T are cut into groups of 32 (one half-wave
// ds_read/ds_write_b32); a group's accesses to edge j of its variables cost
// one LDS cycle per distinct address on the busiest bank (bank = slot mod 32).
// Variables are placed most-constrained first into the first group whose
// banks for all dv edges are still free, then conflicting ones are moved to
// conflict-free groups with room.  Slots are mapped to the kernel's LDS
// positions first (lds_pair_pos).  Padding lanes get dummy positions S + 32 j + f
// (S = lds_pair_span) on banks the group leaves free.
// Measured on a (3,6) n=10000 graph: 3.44 -> ~1.02 cycles per half-wave access
// at T*VPT = 1.126 n.
void build_lane_layout(const HostGraph &h, int T, int VPT, std::vector<int32_t> &lane_var,
                       std::vector<int32_t> &lane_slot) {
    const int n = h.n, dv = h.dv, E = lds_pair_span(h.m, h.dc);
    const int P = T * VPT, G = P / 32;
    std::vector<int> pos((size_t)n * dv), bank((size_t)n * dv);
    std::vector<int> deg((size_t)dv * 32, 0);
    for (int v = 0; v < n; ++v)
        for (int j = 0; j < dv; ++j) {
            pos[(size_t)v * dv + j] = lds_pair_pos(h.vslot[(size_t)v * dv + j], h.dc);
            bank[(size_t)v * dv + j] = pos[(size_t)v * dv + j] & 31;
            deg[(size_t)j * 32 + bank[(size_t)v * dv + j]]++;
        }
    std::vector<int> order(n), score(n);
    for (int v = 0; v < n; ++v) {
        order[v] = v;
        int sc = 0;
        for (int j = 0; j < dv; ++j) sc += deg[(size_t)j * 32 + bank[(size_t)v * dv + j]];
        score[v] = sc;
    }
    std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return score[x] > score[y]; });
    std::vector<int> occ((size_t)G * dv * 32, 0), fill(G, 0), where(n, -1);
    auto conflicts = [&](int q, int v) {
        int c = 0;
        for (int j = 0; j < dv; ++j) c += occ[((size_t)q * dv + j) * 32 + bank[(size_t)v * dv + j]];
        return c;
    };
    auto put = [&](int q, int v, int d) {
        for (int j = 0; j < dv; ++j) occ[((size_t)q * dv + j) * 32 + bank[(size_t)v * dv + j]] += d;
        fill[q] += d;
        where[v] = d > 0 ? q : -1;
    };
    int gi = 0;
    for (int v : order) {
        int best = -1, bestc = 1 << 30;
        for (int k = 0; k < G; ++k) {
            const int q = (gi + k) % G;
            if (fill[q] >= 32) continue;
            const int c = conflicts(q, v);
            if (c < bestc) { bestc = c; best = q; if (c == 0) break; }
        }
        put(best, v, 1);
        gi = (best + 1) % G;
    }
    for (int round = 0; round < 8; ++round) {
        int moved = 0;
        for (int v = 0; v < n; ++v) {
            const int q = where[v];
            put(q, v, -1);
            if (conflicts(q, v) == 0) { put(q, v, 1); continue; }
            int r = -1;
            for (int k = 0; k < G; ++k)
                if (fill[k] < 32 && conflicts(k, v) == 0) { r = k; break; }
            put(r >= 0 ? r : q, v, 1);
            moved += (r >= 0);
        }
        if (!moved) break;
    }
    lane_var.assign(P, -1);
    lane_slot.assign((size_t)P * dv, 0);
    std::vector<int> cursor(G, 0);
    for (int v = 0; v < n; ++v) {
        const int q = where[v], p = q * 32 + cursor[q]++;
        lane_var[p] = v;
        for (int j = 0; j < dv; ++j) lane_slot[(size_t)p * dv + j] = pos[(size_t)v * dv + j];
    }
    for (int q = 0; q < G; ++q) {
        std::vector<char> used((size_t)dv * 32, 0);  // [edge j][bank]
        for (int l = 0; l < cursor[q]; ++l)
            for (int j = 0; j < dv; ++j) used[(size_t)j * 32 + (lane_slot[((size_t)q * 32 + l) * dv + j] & 31)] = 1;
        for (int l = cursor[q]; l < 32; ++l) {
            for (int j = 0; j < dv; ++j) {
                // dummy position E + 32 j + f lands on bank (E + f) mod 32: take a free one
                int f = 0;
                for (int t = 0; t < 32; ++t)
                    if (!used[(size_t)j * 32 + ((E + t) & 31)]) { f = t; break; }
                used[(size_t)j * 32 + ((E + f) & 31)] = 1;
                lane_slot[((size_t)q * 32 + l) * dv + j] = E + 32 * j + f;
            }
        }
    }
}

// Layout of the irregular kernel (bp_irr_kernel, ldpc_internal.hpp): rows of
// 1024 checks, DC = 6 or 8 slots per check (absent slots hold the check rule's
// neutral value), positions k-major so a row's slots are lane-contiguous (LDS
// conflict-free / coalesced in the slab) and whole rows are either in LDS or in
// the slab; variables sorted by degree, every degree class padded to whole
// 64-lane rows so the degree is wave-uniform; padding lanes of a class get
// private dummy positions after the checks'.  Returns false when the graph is
// outside the kernel's range (variable degree > 4, check degree > 8, > 16 rows,
// > 20 variables per thread, positions beyond 16 bits).
bool build_irr_layout(const HostGraph &h, int &VPT, int &KC, int &DC, int &S, int &P,
                      std::vector<int32_t> &lane, std::vector<int32_t> &cdeg) {
    const int T = kIrrT, n = h.n, m = h.m;
    if (h.max_vdeg > 4 || h.max_cdeg > 8 || n <= 0 || m <= 0) return false;
    DC = h.max_cdeg <= 6 ? 6 : 8;
    KC = (m + T - 1) / T;
    if (KC > 16) return false;
    const int PC = KC * DC * T;  // check positions
    std::vector<int> slot_check(h.cvar.size());
    for (int c = 0; c < m; ++c)
        for (int x = h.cptr[c]; x < h.cptr[c + 1]; ++x) slot_check[x] = c;
    auto pos_of = [&](int slot) {
        const int c = slot_check[slot], j = slot - h.cptr[c];
        return ((c / T) * DC + j) * T + (c % T);
    };
    // rows that fit LDS (whole rows; the rest go to the slab)
    const int rows_lds = (int)std::min<size_t>((size_t)KC, kIrrLdsMsgBytes / ((size_t)DC * T * 4));
    std::vector<int> order(n);
    for (int v = 0; v < n; ++v) order[v] = v;
    auto deg = [&](int v) { return h.vptr[v + 1] - h.vptr[v]; };
    // within a degree class, lanes sorted by which of their edges live in the slab:
    // a 64-lane row then mostly takes one side per edge (the other side's path is skipped)
    auto slab_mask = [&](int v) {
        int msk = 0;
        for (int j = 0; j < deg(v); ++j)
            if (slot_check[h.vslot[h.vptr[v] + j]] / T >= rows_lds) msk |= 1 << j;
        return msk;
    };
    std::vector<int> key(n);
    for (int v = 0; v < n; ++v) key[v] = -deg(v) * 64 + slab_mask(v);
    std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return key[x] < key[y]; });
    // lanes: degree classes padded to 64
    std::vector<int> lv;  // var id per lane, -(d+1) for a padding lane of degree d
    for (size_t a = 0; a < order.size();) {
        const int d = deg(order[a]);
        size_t b = a;
        while (b < order.size() && deg(order[b]) == d) lv.push_back(order[b++]);
        while (lv.size() % 64) lv.push_back(-(d + 1));
        a = b;
    }
    const int need = (int)((lv.size() + T - 1) / T);
    VPT = 0;
    for (int v : {1, 2, 5, 10, 20})
        if (v >= need) { VPT = v; break; }
    if (!VPT) return false;
    const int L = T * VPT;
    lane.assign((size_t)3 * L, 0);
    int dummy = PC;
    for (int q = 0; q < L; ++q) {
        int p4[4] = {0xFFFF, 0xFFFF, 0xFFFF, 0xFFFF};
        int var = -1;
        if (q < (int)lv.size() && lv[q] >= 0) {
            var = lv[q];
            for (int j = 0; j < deg(var); ++j) p4[j] = pos_of(h.vslot[h.vptr[var] + j]);
        } else if (q < (int)lv.size()) {
            for (int j = 0; j < -lv[q] - 1; ++j) p4[j] = dummy++;
        }
        lane[q] = var;
        lane[(size_t)L + q] = p4[0] | (p4[1] << 16);
        lane[(size_t)2 * L + q] = p4[2] | (p4[3] << 16);
    }
    P = dummy;
    if (P >= 0xFFFF) return false;
    // whole rows in LDS while they fit (the dummies too when everything fits)
    S = rows_lds == KC && (size_t)P * 4 <= kIrrLdsMsgBytes ? P : rows_lds * DC * T;
    cdeg.assign((size_t)2 * T, 0);
    for (int t = 0; t < T; ++t)
        for (int k = 0; k < KC; ++k) {
            const int c = k * T + t;
            const int d = c < m ? h.cptr[c + 1] - h.cptr[c] : 0;
            cdeg[(size_t)(k >> 3) * T + t] |= d << (4 * (k & 7));
        }
    return true;
}

// Layer schedule of the layered decoder (bp_layer_kernel).  Two checks conflict when they share
// a variable; the rule, in check order throughout:
//   1. first fit: check c takes the lowest layer that holds none of its neighbours (at most
//      max_cdeg (max_vdeg - 1) + 1 layers).  On random graphs this fills the first layers and
//      leaves a tail of nearly empty ones ((3,6) n = 10,000: 883 .. 5 checks), and every layer
//      costs the kernel a barrier and a pass of all its threads whatever it holds;
//   2. balance to the mean: a check of a layer above ceil(m / L) checks moves to the smallest
//      layer below that size which holds none of its neighbours (ties: the lowest), for up to
//      four passes or until one moves nothing.  The number of layers stays first fit's.
// A change of either step changes every layered decode: it gets a new kLayerRule.
const char *const kLayerRule = "first-fit/check-order+balance-to-mean/v1";

// What every schedule needs of a graph: consistent lists, 1 <= check degree <= 32 everywhere, no
// check holding a variable twice
static bool layers_allowed(const HostGraph &h) {
    if (!h.consistent || h.m <= 0 || h.max_cdeg > kLayerMaxD) return false;
    std::vector<int32_t> row;
    for (int c = 0; c < h.m; ++c) {
        if (h.cptr[c + 1] == h.cptr[c]) return false;
        row.assign(h.cvar.begin() + h.cptr[c], h.cvar.begin() + h.cptr[c + 1]);
        std::sort(row.begin(), row.end());
        if (std::adjacent_find(row.begin(), row.end()) != row.end()) return false;
    }
    return true;
}

bool build_layer_schedule(const HostGraph &h, LayerSchedule &S) {
    S = LayerSchedule();
    const int m = h.m, E = (int)h.cvar.size();
    if (!layers_allowed(h)) return false;
    std::vector<int32_t> slot_check(E);
    for (int c = 0; c < m; ++c)
        for (int s = h.cptr[c]; s < h.cptr[c + 1]; ++s) slot_check[s] = c;
    std::vector<int32_t> &layer = S.layer;
    layer.assign(m, -1);
    // check c fits layer l when no other check of its variables is there
    auto fits = [&](int c, int l) {
        for (int s = h.cptr[c]; s < h.cptr[c + 1]; ++s) {
            const int v = h.cvar[s];
            for (int e = h.vptr[v]; e < h.vptr[v + 1]; ++e) {
                const int c2 = slot_check[h.vslot[e]];
                if (c2 != c && layer[c2] == l) return false;
            }
        }
        return true;
    };
    std::vector<int> size;
    for (int c = 0; c < m; ++c) {
        int l = 0;
        while (l < (int)size.size() && !fits(c, l)) ++l;
        if (l == (int)size.size()) size.push_back(0);
        layer[c] = l;
        ++size[l];
    }
    const int L = (int)size.size(), target = (m + L - 1) / L;
    for (int pass = 0; pass < 4; ++pass) {
        int moved = 0;
        for (int c = 0; c < m; ++c) {
            if (size[layer[c]] <= target) continue;
            int best = -1;
            for (int l = 0; l < L; ++l)
                if (size[l] < target && (best < 0 || size[l] < size[best]) && fits(c, l)) best = l;
            if (best < 0) continue;
            --size[layer[c]];
            layer[c] = best;
            ++size[best];
            ++moved;
        }
        if (!moved) break;
    }
    layer_tables(h, S);
    return true;
}

// The tables of a schedule whose layer[] is given (the colouring's above, a quasi-cyclic code's
// block rows below): L, the layers' sizes, and chk / ptr / tab / var in (layer, falling degree,
// id) order.  layer[c] in [0, L) with no layer empty and no two checks of a layer sharing a
// variable is the caller's to ensure.
void layer_tables(const HostGraph &h, LayerSchedule &S) {
    const int m = h.m, E = (int)h.cvar.size();
    const std::vector<int32_t> &layer = S.layer;
    const int L = *std::max_element(layer.begin(), layer.end()) + 1;
    std::vector<int> size(L, 0);
    for (int c = 0; c < m; ++c) ++size[layer[c]];
    S.L = L;
    S.max_layer = *std::max_element(size.begin(), size.end());
    // (layer, falling degree, id) order, and the kernel's tables
    auto deg = [&](int c) { return h.cptr[c + 1] - h.cptr[c]; };
    S.chk.resize(m);
    for (int c = 0; c < m; ++c) S.chk[c] = c;
    std::stable_sort(S.chk.begin(), S.chk.end(), [&](int a, int b) {
        return layer[a] != layer[b] ? layer[a] < layer[b] : deg(a) > deg(b);
    });
    S.ptr.assign(L + 1, 0);
    for (int l = 0; l < L; ++l) S.ptr[l + 1] = S.ptr[l] + size[l];
    S.tab.assign((size_t)L * kLayerTab, 0);
    S.var.resize(E);
    int w = 0;
    for (int l = 0; l < L; ++l) {
        int32_t *row = &S.tab[(size_t)l * kLayerTab];
        for (int j = 0; j <= kLayerMaxD; ++j) {
            row[j] = w;
            for (int q = S.ptr[l]; q < S.ptr[l + 1] && j < deg(S.chk[q]); ++q) S.var[w++] = h.cvar[h.cptr[S.chk[q]] + j];
        }
    }
}

// Quasi-cyclic codes.  The expansion convention is the header's (include/ldpc_mi355x.h,
// ldpc_graph_create_qc): check r Z + i holds variable c Z + (i + s_rc) mod Z for every non-zero
// cell of block row r, in ascending block-column order (the slot order); a variable's checks are
// in ascending check id.
const char *const kQcLayerRule = "qc/block-row/v1";

int host_graph_from_qc(int mb, int nb, int Z, const int32_t *base, HostGraph &h, QcCode &qc) {
    LDPC_REQUIRE(base && mb > 0 && nb > 0, "bad base matrix arguments");
    LDPC_REQUIRE(Z >= 1, "quasi-cyclic code: need Z >= 1");
    LDPC_REQUIRE((int64_t)mb * Z < (1 << 28) && (int64_t)nb * Z < (1 << 28), "quasi-cyclic code: too large");
    std::vector<int> cdeg(nb, 0);
    int64_t cells = 0;
    qc = QcCode();
    qc.row.assign((size_t)mb * kQcRow, 0);
    for (int r = 0; r < mb; ++r) {
        int32_t *row = &qc.row[(size_t)r * kQcRow];
        int d = 0;
        for (int c = 0; c < nb; ++c) {
            const int s = base[(size_t)r * nb + c];
            LDPC_REQUIRE(s >= -1 && s < Z, "quasi-cyclic code: a base entry is -1 (zero block) or a shift in [0, Z)");
            if (s < 0) continue;
            LDPC_REQUIRE(d < kLayerMaxD, "quasi-cyclic code: a block row has more than 32 non-zero blocks");
            row[1 + 2 * d] = c * Z;
            row[2 + 2 * d] = s;
            ++d;
            ++cdeg[c];
        }
        LDPC_REQUIRE(d > 0, "quasi-cyclic code: an all-zero block row");
        row[0] = d;
        cells += d;
    }
    for (int c = 0; c < nb; ++c) LDPC_REQUIRE(cdeg[c] > 0, "quasi-cyclic code: an all-zero block column");
    LDPC_REQUIRE(cells * Z < (1 << 30), "quasi-cyclic code: too many edges");
    qc.Z = Z; qc.mb = mb; qc.nb = nb;
    const int n = nb * Z, m = mb * Z, E = (int)(cells * Z);
    std::vector<int32_t> cptr(m + 1, 0), cvar(E), vptr(n + 1, 0), vslot(E);
    for (int r = 0; r < mb; ++r) {
        const int32_t *row = &qc.row[(size_t)r * kQcRow];
        for (int i = 0; i < Z; ++i) {
            const int c = r * Z + i, e0 = cptr[c];
            cptr[c + 1] = e0 + row[0];
            for (int j = 0; j < row[0]; ++j) {
                const int v = row[1 + 2 * j] + (i + row[2 + 2 * j]) % Z;
                cvar[e0 + j] = v;
                ++vptr[v + 1];
            }
        }
    }
    for (int v = 0; v < n; ++v) vptr[v + 1] += vptr[v];
    std::vector<int32_t> fill(vptr.begin(), vptr.end() - 1);
    for (int e = 0; e < E; ++e) vslot[fill[cvar[e]]++] = e;  // slots ascend with the check id
    return host_graph_from_csr(cptr.data(), cvar.data(), vptr.data(), vslot.data(), n, m, h);
}

void host_layouts(const HostGraph &h, GraphShape &g, HostLayouts &L, bool layouts, const LayoutOptions &opt) {
    g.n = h.n; g.m = h.m; g.k = h.k;
    g.E = (int)h.cvar.size();
    g.dv = h.dv; g.dc = h.dc;
    g.max_vdeg = h.max_vdeg; g.max_cdeg = h.max_cdeg;
    g.consistent = h.consistent;
    g.vchk_len = (int)h.vchk.size();
    if (!layouts || !h.consistent) return;
    int T = 0, VPT = 0;
    if (h.dv == 3 && h.dc == 6 && lds_shape(h.n, T, VPT) &&
        (size_t)(lds_pair_span(h.m, h.dc) + kLdsDummy) * 4 <= 150 * 1024) {
        build_lane_layout(h, T, VPT, L.lane_var, L.lane_slot);
        g.lane_T = T;
        g.lane_VPT = VPT;
    }
    if (LDPC_LOC_LAYOUT && opt.loc_layout) {
        LocLayout &K = L.loc;
        // threads: 256 for up to 1024 check pairs (4 per thread); (3,6) codes up to 2560 pairs:
        // 512 threads x 5 pairs, two workgroups per CU when both fit the LDS (the bench code:
        // +29 % over one 1024-thread workgroup, whose barriers idle the CU); 1024 for up to
        // 3072 (3 per thread: 4 do not fit 128 VGPRs), else 512 threads with 256 VGPRs (up to
        // 10 per thread)
        const int P = h.m / 2;
        const bool r36 = h.dv == 3 && h.dc == 6;
        K.T = P <= 1024 ? 256 : (r36 && P <= 2560 ? 512 : (P <= 3072 ? 1024 : 512));
        if (opt.loc_T) K.T = opt.loc_T;  // shape experiments, ldpc_debug_loc_variant
        bool built = build_loc_layout(h.n, h.m, h.cptr, h.cvar, h.vptr, h.vslot, K);
        if (built && r36 && K.T == 512 && K.KP == 5 && (size_t)std::max(K.words + 64, h.n) * 4 > 80 * 1024) {
            K = LocLayout();  // two workgroups would not fit one CU's LDS
            K.T = 1024;
            built = build_loc_layout(h.n, h.m, h.cptr, h.cvar, h.vptr, h.vslot, K);
        }
        if (built) {
            loc_shape(K, g);
            // the chained layout beside it (the (3,6) 512 x 5 shape only; a graph without one
            // keeps the plain layout for every decode)
            if (LDPC_LOC_CHAIN && opt.loc_chain && loc_variant(g) == kLocReg36 &&
                build_loc_chain_layout(h.n, h.m, h.cptr, h.cvar, h.vptr, h.vslot, K, L.chain)) {
                g.chn_Tq = L.chain.Tq;
                g.chn_words = L.chain.words;
                g.chn_tq = opt.loc_tq;
            } else {
                L.chain = LocChainLayout();
            }
        } else {
            K = LocLayout();
        }
    }
    if (L.lane_var.empty() && LDPC_IRR) {
        int VPT_ = 0, KC = 0, DC = 0, S = 0, P = 0;
        if (build_irr_layout(h, VPT_, KC, DC, S, P, L.irr_lane, L.irr_cdeg)) {
            g.irr_VPT = VPT_; g.irr_KC = KC; g.irr_DC = DC; g.irr_S = S; g.irr_P = P;
        } else {
            L.irr_lane.clear();
            L.irr_cdeg.clear();
        }
    }
    if (opt.qc && opt.qc->Z > 0 && layers_allowed(h)) {
        // a quasi-cyclic code: the block rows are the layers (a block row has at most one
        // circulant per block column, so its Z checks share no variable); all degrees of a block
        // row are equal, so the tables' order is the check order and ptr[l] = l Z
        const QcCode &qc = *opt.qc;
        L.lay = LayerSchedule();
        L.lay.layer.resize(h.m);
        for (int c = 0; c < h.m; ++c) L.lay.layer[c] = c / qc.Z;
        layer_tables(h, L.lay);
        g.lay_L = L.lay.L;
        g.lay_max = L.lay.max_layer;
        g.lay_block_rows = true;
        if (opt.qc_kernel) {
            L.qc_row = qc.row;
            g.qc_Z = qc.Z; g.qc_mb = qc.mb; g.qc_nb = qc.nb;
        }
    } else if (build_layer_schedule(h, L.lay)) {
        g.lay_L = L.lay.L;
        g.lay_max = L.lay.max_layer;
    }
}

}  // namespace ldpc
