// tools/check_geom_edges.cpp — the device headers compiled for the host against the CPU oracle on packed coordinates from a file
// (tests/test_quantiser_edges_host.py writes the quantiser edge sets of tests/quantiser_edges.py into it).  Per structure, every ordered
// residue pair: the accept test (generic form and the squared-distance form with d2_max) and the hash of
//   fd_geom.h        generic chain (fd_pair_feature + fd_hash_enc), shared-subexpression form (fd_pair_both), table form (fd_pair_both_tab,
//                    default 4 angle bins of PDBTrRosetta), and — with the device instructions emulated by tools/host_hip — the speculative
//                    form with and without the squared-distance table (fd_pair_both_spec, fd_dist_bin_tab): whatever it accepts
//   fd_geom_other.h  fd_accept_other / fd_feature_other / fd_hash_other (hash types 2, 4, 5, 6)
// must equal fdo_pair_feature + fdo_hash_any.
//   g++ -O2 -std=c++17 -ffp-contract=off -D__HIPCC__ -Itools/host_hip tools/check_geom_edges.cpp -Loracle -lfdoracle -Wl,-rpath,$PWD/oracle -o check_geom_edges
//   check_geom_edges FILE      FILE: u32 {magic 'FDQE', n_struct, hash_type, nbin_dist, nbin_angle, cutoff (f32 bits), n_res, 0}, u64 res_off[n_struct + 1],
//                              f32 n_xyz[3 n_res], ca_xyz, cb_xyz, u8 aa[n_res]
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../folddisco_amd/csrc/fd_geom_other.h"
#include "../oracle/fd_oracle.h"

// The bin rules, the quantiser factors and (in main) d2_max are RESTATED here from make_consts_bins (csrc/fdgpu_api.hip), which is host code of
// the library and needs the HIP runtime: this tool checks the headers' arithmetic given those constants.  The library's own constants — its
// d2_max correction loops among them — are checked on the device only (tests/test_gpu_quantiser_edges.py: raw lists and index bytes on the
// cutoff edges).  fd_pair_both_spec runs here with v_rsq_f32 / v_sqrt_f32 emulated by correctly rounded values: the device's own
// 1-ulp instructions are exercised by the GPU tests.
static fd_quant make_quant(uint32_t type, uint32_t nbd, uint32_t nba) {
    uint32_t cap_d = 16, def_d = 16, cap_a = 4, def_a = 4;
    if (type == 0) { cap_d = 32; def_d = 18; cap_a = 32; def_a = 9; }
    else if (type == 1) { cap_d = 16; def_d = 8; cap_a = 16; def_a = 3; }
    else if (type == 7) { cap_d = 8; def_d = 8; cap_a = 32; def_a = 32; }
    else if (type == 8) { cap_d = 32; def_d = 32; cap_a = 16; def_a = 16; }
    else if (type == 2) { cap_d = 8; def_d = 8; cap_a = 4; def_a = 3; }
    else if (type == 4 || type == 5) { cap_d = 16; def_d = 8; cap_a = 8; def_a = 3; }
    const bool dflt = nbd == 0 || nba == 0;
    float nd = dflt ? (float)def_d : (nbd > cap_d ? (float)cap_d : (float)nbd);
    float na = dflt ? (float)def_a : (nba > cap_a ? (float)cap_a : (float)nba);
    const float PI_F = 3.14159274f;
    float a_min = -1.0f, a_max = 1.0f;
    if (type == 0) { a_min = 0.0f; a_max = 180.0f; }
    else if (type == 7 || type == 8) { a_min = -PI_F; a_max = PI_F; }
    volatile float cont_d = (20.0f - 2.0f) / (nd - 1.0f);
    volatile float cont_a = (a_max - a_min) / (na - 1.0f);
    float n180 = type == 7 ? fminf(na, 32.0f) : fminf(na, 8.0f);
    volatile float cont_t = (PI_F - 0.0f) / (n180 - 1.0f);
    fd_quant q;
    q.dist_disc = 1.0f / cont_d; q.ang_disc = 1.0f / cont_a; q.ang2_disc = 1.0f / cont_t; q.type = type;
    return q;
}

int main(int argc, char **argv) {
    if (argc < 2) { fprintf(stderr, "usage: %s FILE\n", argv[0]); return 2; }
    FILE *fh = fopen(argv[1], "rb");
    uint32_t hd[8];
    if (!fh || fread(hd, 4, 8, fh) != 8 || hd[0] != 0x45514446u) { fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
    const uint32_t S = hd[1], type = hd[2], nbd = hd[3], nba = hd[4], R = hd[6];
    float cutoff;
    memcpy(&cutoff, &hd[5], 4);
    std::vector<uint64_t> off(S + 1);
    std::vector<float> N(3 * (size_t)R), CA(3 * (size_t)R), CB(3 * (size_t)R);
    std::vector<uint8_t> aa(R), ok(R, 1);
    if (fread(off.data(), 8, S + 1, fh) != S + 1 || fread(N.data(), 4, 3 * (size_t)R, fh) != 3 * (size_t)R || fread(CA.data(), 4, 3 * (size_t)R, fh) != 3 * (size_t)R ||
        fread(CB.data(), 4, 3 * (size_t)R, fh) != 3 * (size_t)R || fread(aa.data(), 1, R, fh) != R) { fprintf(stderr, "short file\n"); return 2; }
    fclose(fh);
    if (fdo_set_hash_type(type) != 0) return 2;
    const fd_quant q = make_quant(type, nbd, nba);
    float d2_max = cutoff * cutoff;      // largest f32 whose sqrt is <= cutoff (make_consts_bins)
    while (sqrtf(d2_max) > cutoff) d2_max = nextafterf(d2_max, 0.0f);
    while (sqrtf(nextafterf(d2_max, INFINITY)) <= cutoff) d2_max = nextafterf(d2_max, INFINITY);
    const bool own = fd_own_descriptor(type), tab_form = type == FD_HASH_PDBTR && q.ang_disc == 1.5f;
    uint32_t tab[FD_BINTAB_WORDS];
    fd_fill_bintab(tab);
    uint32_t tab_f[FD_BINTAB_WORDS];     // the float thresholds of the speculative form, padding clamped to FLT_MAX (k_pair_emit2's prologue)
    for (int k = 0; k < FD_BINTAB_WORDS; ++k) tab_f[k] = tab[k];
    for (int m = 0; m < 4; ++m)
        for (int k = 0; k < 4; ++k) if (tab_f[7 + 5 * m + k] > 0x7f7fffffu) tab_f[7 + 5 * m + k] = 0x7f7fffffu;
    const bool dist_tab = tab_form && q.dist_disc == 1.0f / ((20.0f - 2.0f) / 15.0f);
    long spec_tried = 0, spec_accepted = 0;
    long rev_differ = 0, rev_taken = 0;      // tried pairs on which the oracle's two readings of one dihedral give different keys; those the speculation accepted
    std::vector<uint32_t> off32(off.begin(), off.end());
    fd_batch_view B = {N.data(), CA.data(), CB.data(), aa.data(), ok.data(), off32.data(), nullptr, nullptr, nullptr, S, 0};
    long pairs = 0, accepted = 0, bad = 0;
    for (uint32_t s = 0; s < S; ++s) {
        const uint32_t r0 = off32[s], r1 = off32[s + 1], n = r1 - r0;
        fdo_structure *st = fdo_structure_from_packed((int32_t)n, N.data() + 3 * (size_t)r0, CA.data() + 3 * (size_t)r0, CB.data() + 3 * (size_t)r0, nullptr, aa.data() + r0, nullptr);
        std::vector<fd_frame> F(n);
        for (uint32_t i = 0; i < n; ++i) F[i] = fd_make_frame(fd_load3(N.data(), r0 + i), fd_load3(CA.data(), r0 + i), fd_load3(CB.data(), r0 + i));
        float feat[9], f[FD_NFEAT];
        for (uint32_t i = 0; i < n; ++i)
            for (uint32_t j = 0; j < n; ++j) {
                if (i == j) continue;
                ++pairs;
                const int acc = fdo_pair_feature(st, i, j, cutoff, feat);
                const uint32_t want = acc ? fdo_hash_any(feat, nbd, nba) : 0u;
                accepted += acc;
                const uint32_t gi = r0 + i, gj = r0 + j;
                const char *what = nullptr;
                uint32_t got = 0;
                if (own) {
                    const bool a1 = fd_accept_other(type, B, r0, r1, gi, gj, cutoff), a2 = fd_feature_other(type, B, r0, r1, gi, gj, cutoff, f);
                    if (a1 != (bool)acc || a2 != (bool)acc) what = "accept (fd_geom_other.h)";
                    else if (acc && (got = fd_hash_other(type, f, q)) != want) what = "fd_hash_other";
                } else {
                    const fd_v3 ca1 = fd_load3(CA.data(), gi), ca2 = fd_load3(CA.data(), gj);
                    const bool a1 = !(fd_dist(ca1, ca2) > cutoff), a2 = !(fd_dist2(ca1, ca2) > d2_max);
                    if (a1 != (bool)acc || a2 != (bool)acc) what = a1 != (bool)acc ? "accept (distance)" : "accept (d2_max)";
                    else if (acc) {
                        fd_feature ft = fd_pair_feature(fd_load3(N.data(), gi), ca1, fd_load3(CB.data(), gi), fd_load3(N.data(), gj), ca2, fd_load3(CB.data(), gj));
                        if ((got = fd_hash_enc(aa[gi], aa[gj], ft, q)) != want) what = "generic";
                        uint32_t h_ij, h_ji, want_ji = 0;      // the descriptor's accept test is symmetric: (j, i) is accepted too
                        if (fdo_pair_feature(st, j, i, cutoff, feat)) want_ji = fdo_hash_any(feat, nbd, nba);
                        if (!what) {
                            fd_pair_both(F[i], F[j], aa[gi], aa[gj], q, &h_ij, &h_ji);
                            if ((got = h_ij) != want) what = "shared-subexpression";
                            else if ((got = h_ji) != want_ji) what = "shared-subexpression (second orientation)";
                        }
                        if (!what && tab_form) {
                            fd_pair_both_tab(F[i], F[j], aa[gi], aa[gj], q, tab, &h_ij, &h_ji);
                            if ((got = h_ij) != want) what = "table";
                            else if ((got = h_ji) != want_ji) what = "table (second orientation)";
                        }
                        if (!what && tab_form) {       // speculative torsions: an ACCEPTED result must be the reference's; a refusal takes the table form above
                            ++spec_tried;
                            // tor1(i,j) / tor2(j,i) and tor1(j,i) / tor2(i,j) are one dihedral each, read in both directions (fd_geom.h): the speculation
                            // decides each once, so a pair on which the oracle's two readings differ must be refused
                            const bool differ = ((want >> 4) & 15u) != (want_ji & 15u) || (want & 15u) != ((want_ji >> 4) & 15u);
                            rev_differ += differ;
                            if (fd_pair_both_spec<false>(F[i], F[j], aa[gi], aa[gj], q, tab, tab_f, &h_ij, &h_ji)) {
                                ++spec_accepted;
                                rev_taken += differ;
                                if ((got = h_ij) != want) what = "speculative";
                                else if ((got = h_ji) != want_ji) what = "speculative (second orientation)";
                            }
                            if (!what && dist_tab && fd_pair_both_spec<true>(F[i], F[j], aa[gi], aa[gj], q, tab, tab_f, &h_ij, &h_ji, fd_dist_thr_bits)) {
                                rev_taken += differ;
                                if ((got = h_ij) != want) what = "speculative + distance table";
                                else if ((got = h_ji) != want_ji) what = "speculative + distance table (second orientation)";
                            }
                        }
                    }
                }
                if (what && bad++ < 10) fprintf(stderr, "structure %u pair (%u,%u): %s %08x oracle %08x (accepted %d)\n", s, i, j, what, got, want, acc);
            }
        fdo_structure_free(st);
    }
    printf("type %u bins %u/%u cutoff %g: %u structures, %ld ordered pairs, %ld accepted, speculation %ld of %ld, mismatches: %ld; reversed readings differ on %ld, speculation took %ld of them\n", type, nbd, nba, cutoff, S, pairs, accepted,
           spec_accepted, spec_tried, bad, rev_differ, rev_taken);
    return bad ? 1 : 0;
}
