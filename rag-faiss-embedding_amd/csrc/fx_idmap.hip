// fx_idmap.hip -- stable external ids: faiss's IndexIDMap / IndexIDMap2 on the
// flat index.
//
// A labelled index (fx_index_add_with_ids) carries one caller-chosen int64
// label per row, device-resident next to the rows (FxIndex::labels).  The
// row -> label direction is one load at the writers of I (result_id,
// fx_device.h).  This file is the label -> row direction, all of it streaming
// passes over the label array (8 B per row, each wave instruction 512
// contiguous bytes):
//
//   k_sel_range_lbl / k_sel_bitmap_lbl / k_sel_ids_lbl   a selector's row mask
//                (fx_select.hip) from label membership: one lane per row, a
//                wave's 64 membership bits are two mask words (one ballot, one
//                8-byte store).  The id list of k_sel_ids_lbl is radix-sorted
//                once (hipCUB) and every row binary-searches its label in it;
//                duplicates in the list and ids no row carries cost nothing.
//   k_rows_match / k_rows_scatter   rows_of_ids (IndexIDMap2::rev_map): the
//                query ids are sorted with their positions, every row
//                binary-searches its label and atomicMax-es its row number into
//                the slot of the id's first sorted position (the LAST row of a
//                label wins); the second kernel gives every entry of a run the
//                run's answer and scatters it back to input order.
//   k_compact_labels   remove_ids: kept row r's label goes to slot prefix(r) of
//                a second buffer (out of place: no ordering between workgroups
//                needed), from the prefix words fx_remove.hip computed.
#include "fx_device.h"

#include <hipcub/hipcub.hpp>

#include <algorithm>

namespace fx {

constexpr int IDM_THREADS = 256;
constexpr unsigned IDM_MAX_GRID = 8192;

namespace {

inline size_t idm_align(size_t x) { return (x + 255) & ~(size_t)255; }

unsigned idm_grid(int64_t items) {
    const int64_t g = (items + IDM_THREADS - 1) / IDM_THREADS;
    return (unsigned)std::max<int64_t>(1, std::min<int64_t>(g, IDM_MAX_GRID));
}

}  // namespace

// first position of sorted[0, n) whose value is >= v
__device__ __forceinline__ int64_t idm_lower_bound(const int64_t* __restrict__ sorted, int64_t n, int64_t v) {
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (sorted[mid] < v) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// The mask builders' frame: one lane per row of the mask's sel_mask_words(ntotal)
// * 32 row slots (a multiple of 128, so whole waves), member(label) for rows
// below ntotal, the wave's ballot -> its two mask words.  Slots at or past
// ntotal stay 0 whatever `invert` says.
template <class Member>
__device__ __forceinline__ void idm_build_mask(const int64_t* __restrict__ labels, int64_t ntotal, int invert,
                                               int64_t nwords, uint32_t* __restrict__ mask, Member member) {
    const int64_t slots = nwords * 32, stride = (int64_t)gridDim.x * IDM_THREADS;
    for (int64_t r = (int64_t)blockIdx.x * IDM_THREADS + threadIdx.x; r < slots; r += stride) {
        bool m = false;
        if (r < ntotal) m = member(labels[r]) != (invert != 0);
        const unsigned long long b = __ballot(m);
        if ((threadIdx.x & 63) == 0)  // r is a multiple of 64 here: words r / 32 and r / 32 + 1
            *(uint2*)(mask + (r >> 5)) = make_uint2((uint32_t)b, (uint32_t)(b >> 32));
    }
}

__global__ __launch_bounds__(IDM_THREADS) void k_sel_range_lbl(const int64_t* __restrict__ labels, int64_t imin,
                                                               int64_t imax, int64_t ntotal, int invert,
                                                               int64_t nwords, uint32_t* __restrict__ mask) {
    idm_build_mask(labels, ntotal, invert, nwords, mask, [&](int64_t l) { return l >= imin && l < imax; });
}

// faiss IDSelectorBitmap::is_member: (uint64_t)id >> 3 < n && the id's bit
__global__ __launch_bounds__(IDM_THREADS) void k_sel_bitmap_lbl(const int64_t* __restrict__ labels,
                                                                const uint8_t* __restrict__ bits, int64_t nbytes,
                                                                int64_t ntotal, int invert, int64_t nwords,
                                                                uint32_t* __restrict__ mask) {
    idm_build_mask(labels, ntotal, invert, nwords, mask, [&](int64_t l) {
        const uint64_t byte = (uint64_t)l >> 3;
        return byte < (uint64_t)nbytes && ((bits[byte] >> (int)(l & 7)) & 1) != 0;
    });
}

__global__ __launch_bounds__(IDM_THREADS) void k_sel_ids_lbl(const int64_t* __restrict__ labels,
                                                             const int64_t* __restrict__ sorted, int64_t n,
                                                             int64_t ntotal, int invert, int64_t nwords,
                                                             uint32_t* __restrict__ mask) {
    idm_build_mask(labels, ntotal, invert, nwords, mask, [&](int64_t l) {
        const int64_t j = idm_lower_bound(sorted, n, l);
        return j < n && sorted[j] == l;
    });
}

__global__ __launch_bounds__(IDM_THREADS) void k_idm_iota(int* __restrict__ v, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * IDM_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * IDM_THREADS)
        v[i] = (int)i;
}

// slot[first sorted position of labels[r]] <- max(.., r) for every row r whose label is in the list
__global__ __launch_bounds__(IDM_THREADS) void k_rows_match(const int64_t* __restrict__ labels, int64_t ntotal,
                                                            const int64_t* __restrict__ sorted, int64_t n,
                                                            int* __restrict__ slot) {
    for (int64_t r = (int64_t)blockIdx.x * IDM_THREADS + threadIdx.x; r < ntotal;
         r += (int64_t)gridDim.x * IDM_THREADS) {
        const int64_t l = labels[r];
        const int64_t j = idm_lower_bound(sorted, n, l);
        if (j < n && sorted[j] == l) atomicMax(slot + j, (int)r);
    }
}

// rows[pos[j]] <- the answer of sorted entry j's run (kept at the run's first position)
__global__ __launch_bounds__(IDM_THREADS) void k_rows_scatter(const int64_t* __restrict__ sorted,
                                                              const int* __restrict__ pos,
                                                              const int* __restrict__ slot, int64_t n,
                                                              int64_t* __restrict__ rows) {
    for (int64_t j = (int64_t)blockIdx.x * IDM_THREADS + threadIdx.x; j < n; j += (int64_t)gridDim.x * IDM_THREADS) {
        const int64_t first = idm_lower_bound(sorted, j + 1, sorted[j]);  // <= j
        rows[pos[j]] = (int64_t)slot[first];
    }
}

// one lane per row: a kept row's label -> dst[kept rows before it]
__global__ __launch_bounds__(IDM_THREADS) void k_compact_labels(const int64_t* __restrict__ labels,
                                                                const uint32_t* __restrict__ mask,
                                                                const unsigned* __restrict__ prefix, int64_t ntotal,
                                                                int64_t* __restrict__ dst) {
    for (int64_t r = (int64_t)blockIdx.x * IDM_THREADS + threadIdx.x; r < ntotal;
         r += (int64_t)gridDim.x * IDM_THREADS) {
        const uint32_t keep = ~mask[r >> 5];  // (bits of rows >= ntotal are never looked at: r < ntotal)
        const int b = (int)(r & 31);
        if ((keep >> b) & 1u) dst[(int64_t)prefix[r >> 5] + __popc(keep & ((1u << b) - 1u))] = labels[r];
    }
}

hipError_t launch_sel_range_lbl(const int64_t* labels, int64_t imin, int64_t imax, int64_t ntotal, int invert,
                                uint32_t* mask, hipStream_t s) {
    const int64_t nw = sel_mask_words(ntotal);
    if (nw <= 0) return hipSuccess;
    if (!labels || !mask) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_sel_range_lbl, dim3(idm_grid(nw * 32)), dim3(IDM_THREADS), 0, s, labels, imin, imax, ntotal,
                       invert, nw, mask);
    return hipGetLastError();
}

hipError_t launch_sel_bitmap_lbl(const int64_t* labels, const uint8_t* bits, int64_t nbytes, int64_t ntotal,
                                 int invert, uint32_t* mask, hipStream_t s) {
    const int64_t nw = sel_mask_words(ntotal);
    if (nw <= 0) return hipSuccess;
    if (!labels || !mask || (nbytes > 0 && !bits)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_sel_bitmap_lbl, dim3(idm_grid(nw * 32)), dim3(IDM_THREADS), 0, s, labels, bits, nbytes,
                       ntotal, invert, nw, mask);
    return hipGetLastError();
}

// workspace of the label-side sorts: [sorted ids: n i64 | (pairs: positions in,
// positions sorted, slots: n i32 each) | rocPRIM temporaries]
namespace {

struct IdmCarve {
    size_t sorted = 0, pos_in = 0, pos = 0, slot = 0, temp = 0, temp_bytes = 0, total = 0;
};

hipError_t idm_carve(int64_t n, bool pairs, IdmCarve* c) {
    if (n <= 0 || n > INT_MAX) return hipErrorInvalidValue;
    hipError_t e;
    if (pairs)
        e = hipcub::DeviceRadixSort::SortPairs(nullptr, c->temp_bytes, (const int64_t*)nullptr, (int64_t*)nullptr,
                                               (const int*)nullptr, (int*)nullptr, (int)n, 0, 64, (hipStream_t)0);
    else
        e = hipcub::DeviceRadixSort::SortKeys(nullptr, c->temp_bytes, (const int64_t*)nullptr, (int64_t*)nullptr,
                                              (int)n, 0, 64, (hipStream_t)0);
    if (e != hipSuccess) return e;
    size_t o = 0;
    c->sorted = o;
    o = idm_align(o + (size_t)n * 8);
    if (pairs) {
        c->pos_in = o;
        o = idm_align(o + (size_t)n * 4);
        c->pos = o;
        o = idm_align(o + (size_t)n * 4);
        c->slot = o;
        o = idm_align(o + (size_t)n * 4);
    }
    c->temp = o;
    o = idm_align(o + std::max<size_t>(c->temp_bytes, 16));
    c->total = o;
    return hipSuccess;
}

}  // namespace

hipError_t idmap_sort_bytes(int64_t n, bool pairs, size_t* bytes) {
    IdmCarve c;
    hipError_t e = idm_carve(n, pairs, &c);
    *bytes = c.total;
    return e;
}

hipError_t launch_sel_ids_lbl(const int64_t* labels, const int64_t* ids, int64_t n, int64_t ntotal, int invert,
                              uint32_t* mask, void* ws, size_t ws_bytes, hipStream_t s) {
    const int64_t nw = sel_mask_words(ntotal);
    if (nw <= 0) return hipSuccess;
    if (!labels || !mask) return hipErrorInvalidValue;
    const int64_t* sorted = nullptr;
    if (n > 0) {
        IdmCarve c;
        hipError_t e = idm_carve(n, false, &c);
        if (e != hipSuccess) return e;
        if (!ids || !ws || c.total > ws_bytes) return hipErrorInvalidValue;
        size_t tb = c.temp_bytes;
        e = hipcub::DeviceRadixSort::SortKeys((char*)ws + c.temp, tb, ids, (int64_t*)((char*)ws + c.sorted), (int)n, 0,
                                              64, s);
        if (e != hipSuccess) return e;
        sorted = (const int64_t*)((char*)ws + c.sorted);
    }
    // (an empty list: no row is a member; the search never dereferences `sorted`)
    hipLaunchKernelGGL(k_sel_ids_lbl, dim3(idm_grid(nw * 32)), dim3(IDM_THREADS), 0, s, labels, sorted,
                       n > 0 ? n : (int64_t)0, ntotal, invert, nw, mask);
    return hipGetLastError();
}

hipError_t launch_rows_of_labels(const int64_t* labels, int64_t ntotal, const int64_t* ids, int64_t n, int64_t* rows,
                                 void* ws, size_t ws_bytes, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    IdmCarve c;
    hipError_t e = idm_carve(n, true, &c);
    if (e != hipSuccess) return e;
    if (!ids || !rows || !ws || c.total > ws_bytes || ntotal < 0 || ntotal > INT_MAX || (ntotal > 0 && !labels))
        return hipErrorInvalidValue;
    char* base = (char*)ws;
    int64_t* sorted = (int64_t*)(base + c.sorted);
    int* pos_in = (int*)(base + c.pos_in);
    int* pos = (int*)(base + c.pos);
    int* slot = (int*)(base + c.slot);
    hipLaunchKernelGGL(k_idm_iota, dim3(idm_grid(n)), dim3(IDM_THREADS), 0, s, pos_in, n);
    size_t tb = c.temp_bytes;
    e = hipcub::DeviceRadixSort::SortPairs(base + c.temp, tb, ids, sorted, (const int*)pos_in, pos, (int)n, 0, 64, s);
    if (e != hipSuccess) return e;
    if ((e = hipMemsetAsync(slot, 0xff, (size_t)n * 4, s)) != hipSuccess) return e;  // -1: no row
    if (ntotal > 0)
        hipLaunchKernelGGL(k_rows_match, dim3(idm_grid(ntotal)), dim3(IDM_THREADS), 0, s, labels, ntotal,
                           (const int64_t*)sorted, n, slot);
    hipLaunchKernelGGL(k_rows_scatter, dim3(idm_grid(n)), dim3(IDM_THREADS), 0, s, (const int64_t*)sorted,
                       (const int*)pos, (const int*)slot, n, rows);
    return hipGetLastError();
}

hipError_t launch_compact_labels(const int64_t* labels, const uint32_t* mask, const unsigned* prefix, int64_t ntotal,
                                 int64_t* dst, hipStream_t s) {
    if (ntotal <= 0) return hipSuccess;
    if (!labels || !mask || !prefix || !dst) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_compact_labels, dim3(idm_grid(ntotal)), dim3(IDM_THREADS), 0, s, labels, mask, prefix, ntotal,
                       dst);
    return hipGetLastError();
}

}  // namespace fx
