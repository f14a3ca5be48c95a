// szh_book.h -- part of szhip_kernels.h: the Huffman code book of the SZ 2.1 entropy stage built ON THE DEVICE (opt-in, SZ_HIP_DEV_BOOK=1), so that a Lorenzo-only
// 3-D array's entropy stage is enqueued in one go instead of waiting for the histogram on the host.
//
//   k_huff_book    one workgroup: what szhost_huff_build + szhost_huff_tree_write do (Huffman.c:76-185, :443-585), bit for bit -- the reference's heap order decides
//                  which of two equal counts becomes the left child, so the heap is the reference's heap, sift by sift:
//                    1. leaves in symbol order for the non-zero counts (every thread a contiguous share of the symbols, one scan of the shares' counts);
//                    2. ONE LANE pushes the leaves and merges: the heap's entries are `weight << 16 | node`, so a level of a sift is one LDS read of a child
//                       pair and a compare, the entry on its way down stays in a register; the lane also records every node's parent and subtree size;
//                    3. every thread walks its nodes up to the root (parent links, at most 32 steps): the code word (left = 0, right = 1), its length and the
//                       node's pre-order index (left subtree first: pad_tree, Huffman.c:443-501) -- then the encoder's tables, sum(count x length) and the
//                       serialised tree in one of the reference's node-index widths.
//                  It DECLINES (record.status != 0, nothing else written) an alphabet of more than SZH_BOOK_CAP distinct symbols and a code word of more than 32
//                  bits (the packing passes behind it differ there): the caller builds that book on the host.
//   k_book_tail    the variable tail of the stream header, written where the host would have copied it: intervals, tree size, node count, tree, mean byte /
//                  value, indicator bits, unpredictable count
//   k_book_unpred  the unpredictable values from the encoder's list into the stream (their place and number are the device's)
#pragma once

#define SZH_BOOK_CAP 1024                                    // distinct symbols the LDS heap holds (2 * SZH_BOOK_CAP - 1 nodes: 16-bit links)
#define SZH_BOOK_NODES (2 * SZH_BOOK_CAP)
// status of a record
#define SZH_BOOK_OK 0
#define SZH_BOOK_TOO_MANY 1                                  // more distinct symbols than SZH_BOOK_CAP
#define SZH_BOOK_LONG_CODE 2                                 // a code word of more than 32 bits
#define SZH_BOOK_EMPTY 3                                     // every count is zero
#define SZH_BOOK_TREE_CAP 4                                  // the serialised tree does not fit the caller's buffer
#define SZH_BOOK_STREAM_CAP 5                                // (inside a compress call) the stream or its unpredictable values outgrow the buffers sized before the call
// table layouts
#define SZH_BOOK_TAB_RAW 0                                   // code word right-aligned (k_encode)
#define SZH_BOOK_TAB_E32 1                                   // code << 8 | length (k_encode32)
#define SZH_BOOK_TAB_SEG 2                                   // code << 32 | length, bit 16 set for symbol 0 (k_col_encode)

struct szh_book_rec { unsigned n_nodes, tree_bytes, max_len, status; u64 total_bits, total_unpred; };
// what a compress call's later kernels read instead of host arguments (u64 slots behind the record)
enum { SZH_PLAN_STATUS = 0, SZH_PLAN_BIT0 = 1, SZH_PLAN_HDR_LEN = 2, SZH_PLAN_TOTAL_LEN = 3, SZH_PLAN_COUNT = 4 };

// plan (may be null): plan_fixed = the header's length without the tree, elem = bytes per unpredictable value, stream_cap / unpred_cap = the buffers' sizes
__global__ __launch_bounds__(256) void k_huff_book(const unsigned *__restrict__ hist, unsigned intervals, int layout, unsigned char *__restrict__ tree, unsigned tree_cap,
                                                   u64 *__restrict__ code_tab, uint8_t *__restrict__ len_tab, szh_book_rec *__restrict__ rec,
                                                   u64 *__restrict__ plan, u64 plan_fixed, unsigned elem, u64 stream_cap, u64 unpred_cap)
{
    __shared__ __attribute__((aligned(16))) u64 hp[SZH_BOOK_CAP + 2];         // the heap, entries 1 .. hn: weight << 16 | node
    __shared__ unsigned leaf_w[SZH_BOOK_CAP];                                 // a leaf's count
    __shared__ uint16_t leaf_sym[SZH_BOOK_CAP];
    __shared__ uint16_t lch[SZH_BOOK_NODES], par[SZH_BOOK_NODES], sz[SZH_BOOK_NODES];   // left child; parent (bit 15: this node is its right child); nodes of the subtree
    __shared__ unsigned wsum[4];
    __shared__ unsigned s_maxlen;
    __shared__ u64 s_bits;
    const unsigned tid = threadIdx.x, lane = tid & 63u, wid = tid >> 6;
    // ---- 1. leaves in symbol order
    const unsigned per = (intervals + 255u) / 256u, s_lo = tid * per, s_hi = s_lo + per < intervals ? s_lo + per : intervals;
    unsigned mine = 0;
    for (unsigned s = s_lo; s < s_hi; ++s) mine += hist[s] != 0u ? 1u : 0u;
    unsigned incl = mine;
    for (int o = 1; o < 64; o <<= 1) { const unsigned t = __shfl_up(incl, o, 64); if ((int)lane >= o) incl += t; }
    if (lane == 63u) wsum[wid] = incl;
    if (tid == 0) { s_maxlen = 0u; s_bits = 0ull; }
    __syncthreads();
    unsigned base = incl - mine, D = 0;
    for (unsigned w = 0; w < 4u; ++w) { if (w < wid) base += wsum[w]; D += wsum[w]; }
    const unsigned total = D ? 2u * D - 1u : 0u;
    const unsigned wd = total <= 256u ? 1u : 2u;                              // node-index width of the serialised tree (SZH_BOOK_NODES <= 65536: never four bytes)
    const unsigned tree_bytes = 1u + 2u * wd * total + 5u * total;
    unsigned status = D == 0u ? SZH_BOOK_EMPTY : (D > SZH_BOOK_CAP ? SZH_BOOK_TOO_MANY : (tree_bytes > tree_cap ? SZH_BOOK_TREE_CAP : SZH_BOOK_OK));
    if (status == SZH_BOOK_OK) {
        unsigned k = base;
        for (unsigned s = s_lo; s < s_hi; ++s) {
            const unsigned c = hist[s];
            if (c) { leaf_w[k] = c; leaf_sym[k] = (uint16_t)s; sz[k] = 1; ++k; }
        }
    }
    __syncthreads();
    // ---- 2. the reference's heap, on one lane
    if (status == SZH_BOOK_OK && tid == 0) {
        unsigned hn = 0;
        auto push = [&](u64 key) {
            unsigned i = ++hn;
            while (i > 1u) {
                const u64 pk = hp[i >> 1];
                if ((pk >> 16) <= (key >> 16)) break;
                hp[i] = pk; i >>= 1;
            }
            hp[i] = key;
        };
        auto pop = [&]() -> u64 {
            const u64 top = hp[1], last = hp[hn];
            const unsigned n = --hn;
            if (n >= 1u) {
                unsigned i = 1;
                for (;;) {
                    unsigned c = i << 1;
                    if (c > n) break;
                    u64 kc = hp[c]; const u64 k1 = hp[c + 1];                 // (c is even: the pair is one aligned 16-byte read; hp has a spare entry behind the last)
                    if (c + 1 <= n && (k1 >> 16) < (kc >> 16)) { ++c; kc = k1; }
                    if ((last >> 16) > (kc >> 16)) { hp[i] = kc; i = c; } else break;
                }
                hp[i] = last;
            }
            return top;
        };
        for (unsigned x = 0; x < D; ++x) push(((u64)leaf_w[x] << 16) | x);
        unsigned nn = D;
        while (hn > 1u) {
            const u64 k1 = pop(), k2 = pop();
            const unsigned first = (unsigned)(k1 & 0xffffu), second = (unsigned)(k2 & 0xffffu);
            par[first] = (uint16_t)(nn | 0x8000u);                            // the smaller one: right, bit 1 (Huffman.c:181)
            par[second] = (uint16_t)nn;
            lch[nn] = (uint16_t)second;
            sz[nn] = (uint16_t)(sz[first] + sz[second] + 1u);
            push((((k1 >> 16) + (k2 >> 16)) << 16) | nn);
            ++nn;
        }
        par[total - 1u] = 0x7fffu;                                            // the root (the one leaf of a one-symbol book)
    }
    __syncthreads();
    // ---- 3a. the longest code word
    if (status == SZH_BOOK_OK) {
        unsigned longest = 0;
        for (unsigned x = tid; x < D; x += 256u) {
            unsigned len = 0, p = par[x];
            while (p != 0x7fffu && len <= 32u) { ++len; p = par[p & 0x7fffu]; }
            longest = len > longest ? len : longest;
        }
        if (longest) atomicMax(&s_maxlen, longest);
    }
    __syncthreads();
    const unsigned maxlen = s_maxlen;
    if (status == SZH_BOOK_OK && maxlen > 32u) status = SZH_BOOK_LONG_CODE;
    // ---- 3b. code words, pre-order indices, tables, tree
    if (status == SZH_BOOK_OK) {
        u64 bits = 0;
        unsigned char *const pL = tree + 1, *const pR = pL + (size_t)wd * total, *const pC = pR + (size_t)wd * total, *const pt = pC + (size_t)4 * total;
        if (tid == 0) tree[0] = 0;                                            // "little-endian system"
        for (unsigned x = tid; x < total; x += 256u) {
            unsigned len = 0, pre = 0, p = par[x];
            u64 code = 0;
            while (p != 0x7fffu) {
                const unsigned up = p & 0x7fffu;
                if (p & 0x8000u) { code |= 1ull << len; pre += sz[lch[up]]; }
                ++pre; ++len; p = par[up];
            }
            const bool leaf = x < D;
            const unsigned L = leaf ? 0u : pre + 1u, R = leaf ? 0u : pre + 1u + sz[lch[x]], C = leaf ? leaf_sym[x] : 0u;
            if (wd == 1u) { pL[pre] = (unsigned char)L; pR[pre] = (unsigned char)R; }
            else { pL[2u * pre] = (unsigned char)L; pL[2u * pre + 1u] = (unsigned char)(L >> 8); pR[2u * pre] = (unsigned char)R; pR[2u * pre + 1u] = (unsigned char)(R >> 8); }
            pC[4u * pre] = (unsigned char)C; pC[4u * pre + 1u] = (unsigned char)(C >> 8); pC[4u * pre + 2u] = 0; pC[4u * pre + 3u] = 0;
            pt[pre] = leaf ? 1 : 0;
            if (leaf) {
                code_tab[C] = layout == SZH_BOOK_TAB_SEG ? (code << 32) | len | (C == 0u ? 0x10000u : 0u) : (layout == SZH_BOOK_TAB_E32 ? (code << 8) | len : code);
                len_tab[C] = (uint8_t)len;
                bits += (u64)leaf_w[x] * len;
            }
        }
        // symbols that do not occur: empty entries
        for (unsigned s = s_lo; s < s_hi; ++s)
            if (hist[s] == 0u) { code_tab[s] = layout == SZH_BOOK_TAB_SEG && s == 0u ? 0x10000ull : 0ull; len_tab[s] = 0; }
        if (bits) atomicAdd(&s_bits, bits);
    }
    __syncthreads();
    if (tid == 0) {
        const u64 total_bits = s_bits, total_unpred = intervals ? hist[0] : 0u;
        if (status == SZH_BOOK_OK && plan) {
            const u64 hdr_len = plan_fixed + tree_bytes, unpred_bytes = total_unpred * elem, total_len = hdr_len + unpred_bytes + (total_bits + 7) / 8;
            if (total_len + 64 > stream_cap || unpred_bytes > unpred_cap) status = SZH_BOOK_STREAM_CAP;
            plan[SZH_PLAN_BIT0] = (hdr_len + unpred_bytes) * 8; plan[SZH_PLAN_HDR_LEN] = hdr_len; plan[SZH_PLAN_TOTAL_LEN] = total_len;
        }
        if (plan) plan[SZH_PLAN_STATUS] = status;
        rec->n_nodes = status == SZH_BOOK_OK || status == SZH_BOOK_STREAM_CAP ? total : 0u;
        rec->tree_bytes = status == SZH_BOOK_OK || status == SZH_BOOK_STREAM_CAP ? tree_bytes : 0u;
        rec->max_len = status == SZH_BOOK_OK || status == SZH_BOOK_STREAM_CAP ? maxlen : 0u;
        rec->status = status;
        rec->total_bits = status == SZH_BOOK_OK || status == SZH_BOOK_STREAM_CAP ? total_bits : 0ull;
        rec->total_unpred = total_unpred;
    }
}

// front: the header's fixed front as the host assembled it (front_len bytes), followed by the mean byte and the mean (mid_len bytes); ind: the indicator bits
__global__ __launch_bounds__(256) void k_book_tail(unsigned char *__restrict__ out, const unsigned char *__restrict__ front, unsigned front_len, unsigned mid_len, unsigned intervals,
                                                   const unsigned char *__restrict__ ind, size_t ind_bytes, const unsigned char *__restrict__ tree,
                                                   const szh_book_rec *__restrict__ rec, const u64 *__restrict__ plan)
{
    if (plan[SZH_PLAN_STATUS] != 0) return;
    const unsigned tb = rec->tree_bytes, nn = rec->n_nodes;
    const u64 tu = rec->total_unpred;
    const size_t a = (size_t)front_len + 12, b = a + tb, c = b + mid_len, d = c + ind_bytes, end = d + 8;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < end; i += (size_t)gridDim.x * 256) {
        unsigned char v;
        if (i < front_len) v = front[i];
        else if (i < a) { const unsigned k = (unsigned)(i - front_len), w = k < 4u ? intervals : (k < 8u ? tb : nn); v = (unsigned char)(w >> (24u - 8u * (k & 3u))); }   // big-endian
        else if (i < b) v = tree[i - a];
        else if (i < c) v = front[front_len + (i - b)];
        else if (i < d) v = ind[i - c];
        else v = (unsigned char)(tu >> (8u * (unsigned)(i - d)));             // (the host's own byte order: little-endian)
        out[i] = v;
    }
}

template <class T>
__global__ __launch_bounds__(256) void k_book_unpred(unsigned char *__restrict__ out, const T *__restrict__ unpred, const szh_book_rec *__restrict__ rec, const u64 *__restrict__ plan)
{
    if (plan[SZH_PLAN_STATUS] != 0) return;
    unsigned char *dst = out + plan[SZH_PLAN_HDR_LEN];
    const u64 cnt = rec->total_unpred;
    for (u64 i = (u64)blockIdx.x * 256 + threadIdx.x; i < cnt; i += (u64)gridDim.x * 256) {
        const T v = unpred[i];
        unsigned char b[sizeof(T)];
        memcpy(b, &v, sizeof(T));
#pragma unroll
        for (unsigned k = 0; k < sizeof(T); ++k) dst[i * sizeof(T) + k] = b[k];
    }
}
