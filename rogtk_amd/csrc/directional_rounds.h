// directional_rounds.h — host-side round loop of the directional relaxation.
// Plain C++ with no device types, so that tools/directional_rounds_check.cpp can run it under
// the host sanitizers with a model of the kernel.
#pragma once

#include <cstdint>

namespace rogtk {

constexpr int kDirBatch = 4;  // rounds enqueued between two reads of the "changed" words

// launch(first_round, k): enqueue k <= kDirBatch relaxation rounds; round first_round + j sets
//   word j of the batch when it improves any vertex (the words are cleared by launch).
// read(k, changed): the batch's k words on the host, after the stream has drained.
// A path has at most m - 1 edges, so at most m - 1 rounds improve something and round m
// changes nothing: *rounds = the first round that changed nothing, at most max(m, 1).
// Returns 0; a launch / read error as it came; -1 when round m still changed something
// (never a partial answer: the caller turns it into an error).
template <class Launch, class Read>
int directional_run_rounds(int64_t m, Launch launch, Read read, int64_t* rounds) {
    const int64_t cap = m > 1 ? m : 1;
    int64_t done = 0;
    *rounds = 0;
    while (done < cap) {
        const int k = (int)(cap - done < kDirBatch ? cap - done : kDirBatch);
        if (int rc = launch(done, k)) return rc;
        uint32_t changed[kDirBatch] = {0, 0, 0, 0};
        if (int rc = read(k, changed)) return rc;
        for (int j = 0; j < k; ++j) {
            if (!changed[j]) {
                *rounds = done + j + 1;
                return 0;
            }
        }
        done += k;
    }
    *rounds = done;
    return -1;
}

}  // namespace rogtk
