// fd_verify_host.cpp — fdgpu_verify_host: the index checks of fd_verify.h on host arrays, one list after the other, byte by byte.
// No device and no HIP call: this file also builds with a plain host compiler (and its sanitizers) for runs over hostile input.
#include "fd_verify.h"
#include "fd_postings_host.h"

namespace {
struct vf_part {
    uint64_t n_bad = 0, cls[9] = {0}, first = ~0ull, postings = 0, max_id = 0, max_len = 0;
    void tally(uint64_t slot, uint32_t mask) {
        if (!mask) return;
        ++n_bad;
        for (uint32_t c = 1; c <= 8; ++c) if (mask & FD_VF_BIT(c)) ++cls[c];
        first = std::min(first, slot << 8 | mask);
    }
    void add(const vf_part &o) {
        n_bad += o.n_bad; postings += o.postings;
        for (int c = 0; c < 9; ++c) cls[c] += o.cls[c];
        first = std::min(first, o.first); max_id = std::max(max_id, o.max_id); max_len = std::max(max_len, o.max_len);
    }
};

void table_range(const uint32_t *hashes, const uint64_t *offsets, uint64_t H, uint64_t value_len, uint64_t k0, uint64_t k1, vf_part *out) {
    for (uint64_t k = k0; k < k1; ++k) {      // slots 0 .. H
        uint32_t m = 0;
        if (k == 0 && offsets[0] != 0) m |= FD_VF_BIT(1);
        if (k == H && offsets[H] != value_len) m |= FD_VF_BIT(1);
        if (k < H) {
            if (!(offsets[k] < offsets[k + 1] && offsets[k + 1] <= value_len)) m |= FD_VF_BIT(2);
            else out->max_len = std::max(out->max_len, offsets[k + 1] - offsets[k]);
        }
        if (k + 1 < H && !(hashes[k] < hashes[k + 1])) m |= FD_VF_BIT(3);
        out->tally(k, m);
    }
}

void list_range(const uint64_t *offsets, const uint8_t *value, uint64_t first_id, uint64_t limit, uint64_t k0, uint64_t k1, vf_part *out) {
    for (uint64_t k = k0; k < k1; ++k) {
        const uint64_t b0 = offsets[k], b1 = offsets[k + 1];
        fd_vf_state s = {0, 0};
        uint32_t m = 0, n_term = 0;
        uint64_t sum = 0, first = 0, post = 0;
        for (uint64_t p = b0; p < b1; ++p) {
            uint64_t add;
            uint32_t term;
            m |= fd_vf_byte(&s, value[p], n_term == 0, &add, &term);
            sum = fd_vf_sat(sum + add);
            if (n_term == 0) first += add;
            if (term) { ++post; n_term = 1; }
        }
        m = fd_vf_list_mask(m, value[b1 - 1], first, sum, first_id, limit);
        out->tally(k, m);
        out->postings += post;
        if (!m) out->max_id = std::max(out->max_id, sum);
    }
}

template <typename F>
vf_part run_ranges(uint64_t n, uint32_t n_threads, F f) {
    const uint64_t T = fd_host_threads(n_threads, n, 4096);
    std::vector<vf_part> parts(T);
    fd_over_ranges(T, [&](uint64_t t) { f(n * t / T, n * (t + 1) / T, &parts[t]); });
    vf_part all;
    for (auto &p : parts) all.add(p);
    return all;
}
}      // namespace

// the report from the counters both checkers keep: [0] min of slot << 8 | mask, [1] bad slots, [2..9] classes 1..8, [10] postings, [11] max id, [12] longest list
void fd_vf_fill_report(fd_verify_report *r, const uint64_t cnt[16], uint64_t H, bool list_stage, uint32_t first_hash, uint64_t first_offset) {
    *r = fd_verify_report();
    r->n_bad = cnt[1];
    for (int c = 1; c <= 8; ++c) r->class_count[c] = cnt[1 + c];
    r->list_stage = list_stage ? 1u : 0u;
    r->ok = cnt[1] == 0 ? 1u : 0u;
    if (r->ok) {
        r->n_lists = H; r->n_postings = cnt[10]; r->max_id = cnt[11]; r->max_list_bytes = cnt[12];
    } else {
        r->first_slot = cnt[0] >> 8; r->first_mask = (uint32_t)(cnt[0] & 0xffu); r->first_hash = first_hash; r->first_offset = first_offset;
    }
}

extern "C" int fdgpu_verify_host(const uint32_t *hashes, const uint64_t *offsets, uint64_t H, const uint8_t *value, uint64_t value_len, uint64_t first_id,
                                 uint64_t n_structures, uint32_t n_threads, fd_verify_report *report) {
    if (!report || !offsets || (H && !hashes) || (value_len && !value)) return FDGPU_EINVAL;
    vf_part t = run_ranges(H + 1, n_threads, [&](uint64_t a, uint64_t b, vf_part *o) { table_range(hashes, offsets, H, value_len, a, b, o); });
    const bool lists = t.n_bad == 0;
    if (lists) {
        const uint64_t limit = fd_vf_id_limit(first_id, n_structures);
        vf_part l = run_ranges(H, n_threads, [&](uint64_t a, uint64_t b, vf_part *o) { list_range(offsets, value, first_id, limit, a, b, o); });
        l.max_len = t.max_len;
        t = l;
    }
    const uint64_t cnt[16] = {t.first, t.n_bad, t.cls[1], t.cls[2], t.cls[3], t.cls[4], t.cls[5], t.cls[6], t.cls[7], t.cls[8], t.postings, t.max_id, t.max_len};
    const uint64_t slot = t.n_bad ? t.first >> 8 : 0;
    fd_vf_fill_report(report, cnt, H, lists, t.n_bad && slot < H ? hashes[slot] : 0u, t.n_bad ? offsets[slot] : 0);
    return FDGPU_OK;
}
