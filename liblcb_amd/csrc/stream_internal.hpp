// stream_internal.hpp — shared by stream_kernels.hip and
// lcb_hash_stream_gpu.cpp (liblcb_hash_stream_gpu.so).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace lcbstream {

// Device-side description of one call on a stream set.
struct StreamArgs {
    uint32_t* ctx = nullptr;          // word k of stream s at ctx[k * pitch + s] (stream_state.hpp)
    uint64_t pitch = 0;
    uint32_t nstreams = 0;
    uint32_t words = 0;               // context words of the set's algorithm
    const uint32_t* init = nullptr;   // `words` words: a freshly initialised context
    const uint32_t* opad = nullptr;   // keyed set: the state after K ^ opad (as the context's h | N | Sigma), else nullptr
    const uint32_t* index = nullptr;  // stream of entry i (nullptr: i)
    uint64_t count = 0;
    // update: the chunks
    const uint8_t* data = nullptr;
    const uint64_t* offsets = nullptr;   // nullptr: i * stride
    const uint32_t* lengths = nullptr;   // nullptr: fixed_len
    uint64_t stride = 0;
    uint32_t fixed_len = 0;
    // final
    uint8_t* digests = nullptr;
    uint32_t keep = 0;
    // The index check's verdict: the call stores nothing when *bad == epoch.
    uint32_t* bad = nullptr;             // nullptr: no index list to check
    uint32_t epoch = 0;
    uint32_t* stamp = nullptr;           // one word per stream: the epoch of the last call that listed it
};

// K ^ ipad / K ^ opad mid-states of a keyed set, and the initial context of
// any set: init (a.words words), opad (48 words).  key: device memory.
void launch_stream_prep(int alg, const uint8_t* key, uint64_t key_len, bool keyed, uint32_t* init, uint32_t* opad,
                        hipStream_t s);
// *bad = epoch when index[0..count) holds an index >= nstreams or one twice
// (epochs are never reused, so *bad needs no reset between calls).
void launch_stream_check(const StreamArgs& a, hipStream_t s);
void launch_stream_fill(const StreamArgs& a, hipStream_t s);      // reset
void launch_stream_update(int alg, const StreamArgs& a, hipStream_t s);
void launch_stream_final(int alg, const StreamArgs& a, hipStream_t s);
// Export / import: image = count x words words, entry-major.
void launch_stream_gather(const StreamArgs& a, uint32_t* image, hipStream_t s);
void launch_stream_scatter(const StreamArgs& a, const uint32_t* image, hipStream_t s);

}  // namespace lcbstream
