// persist_plan.h -- the host arithmetic of moving chunk images between HBM and
// chunk files (persist_host.hip): how a batch of files is cut into rounds of
// the device stage, where a file lies in its round, and how large the file of
// a stored image is.  No HIP type: host text only, run stand-alone under ASan
// + UBSan by tools/persist_check.cpp (`make persistcheck`).  Not installed.
#ifndef CIOA_PERSIST_PLAN_H
#define CIOA_PERSIST_PLAN_H

#include <stddef.h>
#include <stdint.h>

namespace cioa {

constexpr uint64_t kPersistAlign = 128;                // a file's slot in the stage: its size rounded up to this
constexpr uint32_t kPersistNoRound = 0xffffffffu;      // round_of: the file is larger than the round maximum
constexpr uint64_t kPersistPageMax = 1ull << 30;       // the largest `page` of a trimmed store
constexpr int kPersistThreads = 16;                    // host threads of a round's reads or writes

// The stage is used whole: one round may fill all of it, down to a multiple of
// the slot alignment.  This is also the largest file a round takes.
inline uint64_t persist_round_max(uint64_t stage_bytes)
{
    return stage_bytes & ~(kPersistAlign - 1);
}

// A file's slot in the stage.  size <= persist_round_max(...): no wrap.
inline uint64_t persist_slot(uint64_t size)
{
    return (size + (kPersistAlign - 1)) & ~(kPersistAlign - 1);
}

// The partition: files in order; a round is a maximal run of consecutive files
// whose slots fit the round maximum.  A file larger than the maximum gets
// kPersistNoRound and closes the round before it.  An empty file takes no
// bytes and rides in the round that is open (it opens one when none is).
// Returns the number of rounds.
inline uint32_t persist_rounds(const uint64_t *sizes, size_t n, uint64_t stage_bytes, uint32_t *round_of)
{
    const uint64_t room = persist_round_max(stage_bytes);
    uint32_t rounds = 0;
    uint64_t used = 0;
    bool open = false;
    for (size_t i = 0; i < n; ++i) {
        if (sizes[i] > room) {
            round_of[i] = kPersistNoRound;
            open = false;
            continue;
        }
        const uint64_t slot = persist_slot(sizes[i]);
        if (!open || slot > room - used) {
            ++rounds;
            used = 0;
            open = true;
        }
        round_of[i] = rounds - 1;
        used += slot;
    }
    return rounds;
}

// The size of the file of a stored image of `used` bytes in a slot of `cap`
// (used <= cap): the capacity untrimmed -- the reference's file is as large as
// its map -- and, trimmed, the used bytes rounded up to page, a power of two
// (1: exact), as cio_file_sync under CIO_TRIM_FILES rounds to the page.
inline uint64_t persist_file_size(uint64_t used, uint64_t cap, bool trim, uint64_t page)
{
    if (!trim) {
        return cap;
    }
    const uint64_t up = used + (page - 1);
    return up < used ? used : up & ~(page - 1);
}

}  // namespace cioa

#endif
