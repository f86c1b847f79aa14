// k_rebase.hip — device-side move of a resident index to another structure id range (fdgpu_index_rebase): the same structures with ids
// new_first_id .. new_first_id + n_structures - 1, byte for byte the build over them with first_id = new_first_id.
//
// A posting list stores its first id as an absolute varint and every later id as a delta (fd_postings.h), so a shift of all ids rewrites the first
// varint of every list and nothing else; its length changes by up to four bytes either way and every list behind it moves.
//
//   k_rb_sizes   thread per list: the first varint (value f, nf bytes), head = f + shift, new length = old - nf + fd_varint_len(head); the last id
//                shifted when the source carries last ids.  Every offset and head is checked here, before anything is written: error bits, no copy
//   scan         the shared exclusive scan over the sizes, straight into the new offsets
//   k_rb_copy    eight lanes per list (fd_list_copy): the head's new varint, then the bytes behind the old one
// HBM-bound byte work: one read + one write of the value bytes, one 8-byte read per list, 25 bytes per hash of tables.
// Workspace: 9 bytes per list — see DESIGN.md §4c.
#include "fdgpu_internal.h"
#include "fd_api_common.h"
#include "fd_postings.h"

struct rb_args { const uint64_t *offsets; const uint8_t *value; const uint32_t *last_ids; uint64_t H, value_len, S; uint32_t first_id, shift; };

// ---- sizes: thread per list.  Reads offsets[t], offsets[t + 1] and, only for b0 < b1 <= value_len, the 8 bytes at value + b0 (FD_VALUE_SLACK).
// A bad list gets size 0 and an error bit: the call fails after this kernel, the copy never runs.
__global__ __launch_bounds__(256) void k_rb_sizes(rb_args A, uint32_t *__restrict__ sizes, uint32_t *__restrict__ heads, uint8_t *__restrict__ nfdl,
                                                  uint32_t *__restrict__ out_last, uint32_t *__restrict__ err) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= A.H) return;
    const uint64_t b0 = A.offsets[t], b1 = A.offsets[t + 1];
    uint32_t sz = 0, head = 0, nf = 0, dl = 0, bad = 0;
    if (b1 <= b0 || b1 > A.value_len) bad = FD_IXERR_DAMAGED;
    else {
        const uint32_t f = fd_first_varint(A.value + b0, &nf);
        uint64_t loc;
        // nf == 0: no terminator in five bytes.  A head below first_id (the downward shift would wrap) or past the last id (the upward one would)
        if (nf == 0 || nf > b1 - b0 || !fd_id_local(f, A.first_id, A.S, &loc)) bad = FD_IXERR_DAMAGED;
        else {
            head = f + A.shift;      // modulo 2^32: shift = new_first_id - first_id; in range because f is and new_first_id + S <= 2^32
            dl = fd_varint_len(head);
            const uint64_t len = b1 - b0 - nf + dl;
            if (len > 0xffffffffull) bad = FD_IXERR_LONG;
            else sz = (uint32_t)len;
        }
    }
    if (bad) atomicOr(err, bad);
    sizes[t] = sz;
    heads[t] = head;
    nfdl[t] = (uint8_t)(bad ? 0u : nf | (dl << 4));
    if (out_last) out_last[t] = A.last_ids[t] + A.shift;
}

// ---- copy: eight lanes per list; launched only after k_rb_sizes found every list sound
__global__ __launch_bounds__(256) void k_rb_copy(rb_args A, const uint32_t *__restrict__ heads, const uint8_t *__restrict__ nfdl,
                                                 const uint64_t *__restrict__ out_off, uint8_t *__restrict__ out_value) {
    const uint64_t t = (uint64_t)blockIdx.x * 32u + (threadIdx.x >> 3);
    if (t >= A.H) return;
    const uint32_t c = nfdl[t], nf = c & 15u, dl = c >> 4;
    const uint64_t b0 = A.offsets[t], b1 = A.offsets[t + 1];
    fd_list_copy(out_value + out_off[t], heads[t], dl, A.value + b0 + nf, b1 - b0 - nf, threadIdx.x & 7u);
}

static int rebase_impl(fdgpu_ctx *c, const fdgpu_index *ix, uint64_t new_first_id, fdgpu_index **out) {
    reset_timings(c);
    hipStream_t st = c->stream;
    const uint64_t H = ix->n_hashes;
    const bool with_last = ix->last_ids != nullptr;      // a loaded index carries none: neither does its rebased copy (fd_index_last_ids makes them on demand)
    fdgpu_index *nx = nullptr;
    if (int rc = fd_index_new(c, true, H, H ? FD_VALUE_LATER : 0, with_last && H, &nx)) return rc;
    *out = nx;
    nx->n_postings = ix->n_postings; nx->n_structures = ix->n_structures; nx->first_id = new_first_id;
    if (!H) {
        HIPCHK(c, hipMemsetAsync(nx->offsets, 0, 8, st));
        HIPCHK(c, hipStreamSynchronize(st));
        return FDGPU_OK;
    }
    HIPCHK(c, c->ws[WS_MISC0].ensure(H * 4));      // new byte length of every list
    HIPCHK(c, c->ws[WS_MISC1].ensure(H * 4));      // its new head
    HIPCHK(c, c->ws[WS_MISC2].ensure(H));          // bytes of the old head's varint | bytes of the new one << 4
    HIPCHK(c, c->ws[WS_SCANTMP].ensure(fd_scan_tmp_elems(H) * 8 + 64));
    HIPCHK(c, c->ws[WS_TOTAL].ensure(64));         // [0] scan total, [1] error bits
    uint32_t *sizes = c->ws[WS_MISC0].as<uint32_t>(), *heads = c->ws[WS_MISC1].as<uint32_t>();
    uint8_t *nfdl = c->ws[WS_MISC2].as<uint8_t>();
    uint64_t *tot = c->ws[WS_TOTAL].as<uint64_t>();
    rb_args A{ix->offsets, ix->value, ix->last_ids, H, ix->value_len, ix->n_structures, (uint32_t)ix->first_id, (uint32_t)(new_first_id - ix->first_id)};
    {
        StageTimer t(c, "rebase_sizes", H * (16 + 8 + 9 + 8 + (with_last ? 8 : 0)) + H * 4);
        HIPCHK(c, hipMemsetAsync(tot, 0, 16, st));
        hipLaunchKernelGGL(k_rb_sizes, dim3(fd_grid(H, 256)), dim3(256), 0, st, A, sizes, heads, nfdl, nx->last_ids, (uint32_t *)(tot + 1));
        fd_exclusive_scan<uint32_t>(sizes, H, nx->offsets, c->ws[WS_SCANTMP].as<uint64_t>(), tot, st);
        HIPCHK(c, hipMemcpyAsync(nx->hashes, ix->hashes, H * 4, hipMemcpyDeviceToDevice, st));
    }
    HIPCHK(c, hipGetLastError());
    uint64_t hv[2] = {0, 0};      // new value length, error bits
    HIPCHK(c, hipMemcpyAsync(hv, tot, sizeof hv, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    if (hv[1] & FD_IXERR_DAMAGED)
        FAIL(c, FDGPU_EINVAL, "index rebase: the index is damaged (offsets that do not ascend inside the value bytes, or a list whose first id is outside "
                              "[first_id, first_id + n_structures))");
    if (hv[1] & FD_IXERR_LONG) FAIL(c, FDGPU_ERANGE, "index rebase: a posting list reaches 4 GiB");
    nx->value_len = hv[0];
    HIPCHK(c, fd_index_block(c, hv[0] + FD_VALUE_SLACK, (void **)&nx->value, &nx->cap_value));
    {
        StageTimer t(c, "rebase_copy", ix->value_len + hv[0] + H * (16 + 8 + 5));
        hipLaunchKernelGGL(k_rb_copy, dim3(fd_grid(H, 32)), dim3(256), 0, st, A, heads, nfdl, nx->offsets, nx->value);
    }
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(st));      // the result is complete, and the context's workspaces free again, when the call returns
    return FDGPU_OK;
}

extern "C" int fdgpu_index_rebase(fdgpu_ctx *c, const fdgpu_index *ix, uint64_t new_first_id, fdgpu_index **out) { FD_LOCK(c);
    if (!c || !ix || !out) return FDGPU_EINVAL;
    *out = nullptr;
    if (new_first_id > 0xffffffffull || new_first_id + ix->n_structures > 0xffffffffull) FAIL(c, FDGPU_ERANGE, "structure ids exceed 32 bits");
    fdgpu_index *nx = nullptr;
    const int rc = rebase_impl(c, ix, new_first_id, &nx);
    if (rc != FDGPU_OK) return fd_index_op_failed(c, rc, &nx);
    *out = nx;
    return FDGPU_OK;
}
