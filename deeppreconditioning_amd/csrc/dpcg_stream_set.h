// The streams of a batch: created one by one, synchronised and destroyed on every way out of the scope -- also when creating them
// fails half-way.  Names no header of its own: whoever includes it has hipStream_t, the three stream calls and DPCG_HIP in scope
// (dpcg_solve.hip: HIP's; tools/stream_set_check.cpp: counting stubs, so that the holder is checked on a CPU build).
#pragma once

#include <vector>

struct StreamSet {
    std::vector<hipStream_t> s;
    StreamSet() = default;
    StreamSet(const StreamSet &) = delete;
    StreamSet &operator=(const StreamSet &) = delete;
    int create(int count) {
        s.reserve((size_t)count);              // (no reallocation between a stream's creation and its place in the list)
        for (int i = 0; i < count; ++i) {
            hipStream_t st = nullptr;
            DPCG_HIP(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
            s.push_back(st);
        }
        return 0;
    }
    ~StreamSet() {
        for (hipStream_t st : s) {
            (void)hipStreamSynchronize(st);
            (void)hipStreamDestroy(st);
        }
    }
};
