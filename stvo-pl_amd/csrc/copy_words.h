// copy_words.h — a workgroup's copy of a run of 8- or 16-byte words with several loads in flight per lane (track_kernel.hip: a
// key-frame set; stream_snapshot.hip: a stream's sections), and the fill that goes with it.  Plain vector loads and stores.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

namespace stvo {

// Words [first_word, first_word + n_words) of `src` to the same words of `dst`, lane `tid` of a workgroup of BLOCK.
template <typename W, int BLOCK>
__device__ __forceinline__ void copy_words(const void* __restrict__ src, void* __restrict__ dst, size_t first_word, int n_words, int tid) {
    const W* s = reinterpret_cast<const W*>(src) + first_word;
    W* d = reinterpret_cast<W*>(dst) + first_word;
    int i = tid;
    for (; i + 3 * BLOCK < n_words; i += 4 * BLOCK) {  // four loads in flight per lane: the copy is a latency chain otherwise
        const W w0 = s[i], w1 = s[i + BLOCK], w2 = s[i + 2 * BLOCK], w3 = s[i + 3 * BLOCK];
        d[i] = w0;
        d[i + BLOCK] = w1;
        d[i + 2 * BLOCK] = w2;
        d[i + 3 * BLOCK] = w3;
    }
    for (; i < n_words; i += BLOCK) d[i] = s[i];
}

// Words [first_word, first_word + n_words) of `dst` become `v`.
template <typename W, int BLOCK>
__device__ __forceinline__ void fill_words(void* __restrict__ dst, size_t first_word, int n_words, W v, int tid) {
    W* d = reinterpret_cast<W*>(dst) + first_word;
    for (int i = tid; i < n_words; i += BLOCK) d[i] = v;
}

}  // namespace stvo
