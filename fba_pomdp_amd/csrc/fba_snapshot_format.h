// fba_snapshot_format.h -- the byte format of a belief snapshot block (fba_belief_export / fba_belief_import, include/fba_hip.h) and the
// host pass of an import: everything that can be said about a block from its 64-byte header alone.  Header-only and free of HIP, so a host
// program that only stores or ships blocks can include it, and so that the checks run under a host sanitizer on their own.
//
//   block  = fba_snapshot_head (64 bytes) | weights: particles * 8 bytes (weighted filters only) | records: particles * particle_bytes
//   records stand from the start of their part at `stride` bytes (64, 128 or particle_bytes for history records, particle_bytes otherwise);
//   every byte behind the last record, behind a history record's last entry and behind a record's state word is zero.
//   checksum = sum over the 32-bit words w[i] of the payload (everything behind the header, i from 0) of w[i] * ((i + 1) * FBA_SNAPSHOT_CHECK_MUL),
//   all in arithmetic modulo 2^64: a sum, so the order of the additions cannot matter.
#pragma once

#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "fba_hip.h"

namespace fba_snapshot {

// words between the records of a slot whose history records hold `total` entries (hist_stride of fba_device.h, in bytes)
inline int64_t history_stride_bytes(int64_t particle_bytes, int total, bool compact)
{
    if (!compact) return particle_bytes;
    const int64_t need = 8 + 4 * (int64_t)total;
    if (need <= 64 && particle_bytes > 64) return 64;
    if (need <= 128 && particle_bytes > 128) return 128;
    return particle_bytes;
}
inline int history_total(uint32_t hist_cnt) { return (int)((hist_cnt & 0xffu) + ((hist_cnt >> 8) & 0xffu) + ((hist_cnt >> 16) & 0xffu) + (hist_cnt >> 24)); }

inline int64_t block_bytes(int weighted, int64_t particles, int64_t particle_bytes)
{
    return (int64_t)sizeof(fba_snapshot_head) + (weighted ? particles * 8 : 0) + particles * particle_bytes;
}

inline uint64_t check_factor(uint64_t index) { return (index + 1) * FBA_SNAPSHOT_CHECK_MUL; }
// the checksum of a payload of `words` 32-bit words (any alignment)
inline uint64_t checksum(const void* payload, uint64_t words)
{
    const unsigned char* p = static_cast<const unsigned char*>(payload);
    uint64_t sum = 0;
    for (uint64_t i = 0; i < words; ++i) {
        uint32_t w;
        memcpy(&w, p + i * 4, 4);
        sum += (uint64_t)w * check_factor(i);
    }
    return sum;
}
// the prior hash: FNV-1a over 32-bit words, continued from `h` (start: FBA_SNAPSHOT_HASH_SEED)
inline uint64_t hash_words(uint64_t h, const void* data, uint64_t words)
{
    const unsigned char* p = static_cast<const unsigned char*>(data);
    for (uint64_t i = 0; i < words; ++i) {
        uint32_t w;
        memcpy(&w, p + i * 4, 4);
        h = (h ^ w) * 0x100000001b3ull;
    }
    return h;
}

// What a context takes: its own fingerprint as a header (hist_cnt, stride, updates and checksum unused), the entries its history records
// have room for, and whether it stores short histories at the short strides.
struct Accepts {
    fba_snapshot_head want;
    int32_t hist_cap;
    int32_t compact;
};

// The host pass over one block of which `avail` bytes are readable.  0 = the header is one this context can take; -1 = refused, with the
// field and both values in msg.  Reads nothing behind min(avail, 64) bytes and nothing of the payload.
inline int check_head(const void* block, int64_t avail, const Accepts& acc, char* msg, size_t msg_len)
{
    const fba_snapshot_head& w = acc.want;
    const int64_t per_slot = block_bytes(w.weighted, w.particles, w.particle_bytes);
    if (!block || avail < per_slot) {
        snprintf(msg, msg_len, "bytes %lld / %lld", (long long)(block ? avail : 0), (long long)per_slot);
        return -1;
    }
    fba_snapshot_head h;
    memcpy(&h, block, sizeof h);
#define FBA_SNAP_FIELD(field, name)                                                                                           \
    if (h.field != w.field) {                                                                                                 \
        snprintf(msg, msg_len, name " %lld in the block, %lld in this context", (long long)h.field, (long long)w.field);      \
        return -1;                                                                                                            \
    }
    if (h.magic != FBA_SNAPSHOT_MAGIC) {
        snprintf(msg, msg_len, "magic 0x%08x / 0x%08x: not a belief snapshot", (unsigned)h.magic, (unsigned)FBA_SNAPSHOT_MAGIC);
        return -1;
    }
    if (h.version != FBA_SNAPSHOT_VERSION) {
        snprintf(msg, msg_len, "layout version %d / %d", (int)h.version, (int)FBA_SNAPSHOT_VERSION);
        return -1;
    }
    FBA_SNAP_FIELD(record_format, "record format")
    FBA_SNAP_FIELD(weighted, "weighted")
    FBA_SNAP_FIELD(model, "model")
    FBA_SNAP_FIELD(domain, "domain")
    FBA_SNAP_FIELD(size, "size")
    FBA_SNAP_FIELD(width, "width")
    FBA_SNAP_FIELD(height, "height")
    if (h.particles != w.particles) {
        snprintf(msg, msg_len, "particles %d / %d", (int)h.particles, (int)w.particles);
        return -1;
    }
    FBA_SNAP_FIELD(particle_bytes, "particle bytes")
    FBA_SNAP_FIELD(counts_len, "counts length")
    FBA_SNAP_FIELD(states, "states")
    FBA_SNAP_FIELD(actions, "actions")
    FBA_SNAP_FIELD(observations, "observations")
#undef FBA_SNAP_FIELD
    if (h.prior_hash != w.prior_hash) {
        snprintf(msg, msg_len, "prior hash %016llx in the block, %016llx in this context: the records stand over another prior",
                 (unsigned long long)h.prior_hash, (unsigned long long)w.prior_hash);
        return -1;
    }
    const bool hist = w.record_format >= 5;
    if (!hist) {
        if (h.hist_cnt != 0) {
            snprintf(msg, msg_len, "hist_cnt 0x%08x / 0: record format %d has no history entries", (unsigned)h.hist_cnt, (int)w.record_format);
            return -1;
        }
        if ((int64_t)h.stride != (int64_t)w.particle_bytes) {
            snprintf(msg, msg_len, "record stride %u / %d", (unsigned)h.stride, (int)w.particle_bytes);
            return -1;
        }
        return 0;
    }
    for (int a = w.actions; a < 4; ++a)
        if ((h.hist_cnt >> (8 * a)) & 0xffu) {
            snprintf(msg, msg_len, "hist_cnt 0x%08x: entries of action %d, the context has %d actions", (unsigned)h.hist_cnt, a, (int)w.actions);
            return -1;
        }
    const int total = history_total(h.hist_cnt);
    if (w.actions > 4 || total > acc.hist_cap) {
        snprintf(msg, msg_len, "hist_cnt 0x%08x: %d entries per record / room for %d", (unsigned)h.hist_cnt, total, (int)acc.hist_cap);
        return -1;
    }
    const int64_t stride = history_stride_bytes(w.particle_bytes, total, acc.compact != 0);
    if ((int64_t)h.stride != stride) {
        snprintf(msg, msg_len, "record stride %u / %lld for %d entries per record", (unsigned)h.stride, (long long)stride, total);
        return -1;
    }
    return 0;
}

// The host pass of fba_belief_convert over one source block of which `avail` bytes are readable: the block of a context that may differ
// from the destination `acc` in two fields only -- particles (every format) and particle_bytes (history formats 5..7, where it is the room
// of a record: particle_bytes / 4 - 2 entries).  src_particles and src_particle_bytes are what all blocks of the call share, those of its
// first block; every other fingerprint field must be the destination's.  hist_cnt and stride are judged against the SOURCE's room with
// history_stride_bytes, as check_head judges them against a context's.  0 = the block can be refitted, and *dst_stride (if asked for) is the
// stride its records take in the destination; -1 = refused, field and both values in msg; -2 = refused because its records hold more entries
// than the destination has room for ("holds t entries per record / room for hist_cap").  Reads nothing behind min(avail, 64) bytes.
inline int check_convert_head(const void* block, int64_t avail, const Accepts& acc, int32_t src_particles, int32_t src_particle_bytes, char* msg, size_t msg_len,
                              int64_t* dst_stride = nullptr)
{
    const fba_snapshot_head& w = acc.want;
    if (!block || avail < (int64_t)sizeof(fba_snapshot_head)) {
        snprintf(msg, msg_len, "bytes %lld / %lld: not even a header", (long long)(block ? avail : 0), (long long)sizeof(fba_snapshot_head));
        return -1;
    }
    fba_snapshot_head h;
    memcpy(&h, block, sizeof h);
#define FBA_SNAP_FIELD(field, name)                                                                                           \
    if (h.field != w.field) {                                                                                                 \
        snprintf(msg, msg_len, name " %lld in the block, %lld in this context", (long long)h.field, (long long)w.field);      \
        return -1;                                                                                                            \
    }
    if (h.magic != FBA_SNAPSHOT_MAGIC) {
        snprintf(msg, msg_len, "magic 0x%08x / 0x%08x: not a belief snapshot", (unsigned)h.magic, (unsigned)FBA_SNAPSHOT_MAGIC);
        return -1;
    }
    if (h.version != FBA_SNAPSHOT_VERSION) {
        snprintf(msg, msg_len, "layout version %d / %d", (int)h.version, (int)FBA_SNAPSHOT_VERSION);
        return -1;
    }
    FBA_SNAP_FIELD(record_format, "record format")
    FBA_SNAP_FIELD(weighted, "weighted")
    FBA_SNAP_FIELD(model, "model")
    FBA_SNAP_FIELD(domain, "domain")
    FBA_SNAP_FIELD(size, "size")
    FBA_SNAP_FIELD(width, "width")
    FBA_SNAP_FIELD(height, "height")
    const bool hist = w.record_format >= 5;
    if (h.particles < 1) {
        snprintf(msg, msg_len, "particles %d: a filter has one particle at least", (int)h.particles);
        return -1;
    }
    if (h.particles != src_particles) {
        snprintf(msg, msg_len, "particles %d in the block, %d in the first block of the call", (int)h.particles, (int)src_particles);
        return -1;
    }
    if (!hist) FBA_SNAP_FIELD(particle_bytes, "particle bytes")
    if (h.particle_bytes < (hist ? 8 : 4) || (h.particle_bytes & 3)) {
        snprintf(msg, msg_len, "particle bytes %d: not a record of whole words", (int)h.particle_bytes);
        return -1;
    }
    if (h.particle_bytes != src_particle_bytes) {
        snprintf(msg, msg_len, "particle bytes %d in the block, %d in the first block of the call", (int)h.particle_bytes, (int)src_particle_bytes);
        return -1;
    }
    FBA_SNAP_FIELD(counts_len, "counts length")
    FBA_SNAP_FIELD(states, "states")
    FBA_SNAP_FIELD(actions, "actions")
    FBA_SNAP_FIELD(observations, "observations")
#undef FBA_SNAP_FIELD
    if (h.prior_hash != w.prior_hash) {
        snprintf(msg, msg_len, "prior hash %016llx in the block, %016llx in this context: the records stand over another prior",
                 (unsigned long long)h.prior_hash, (unsigned long long)w.prior_hash);
        return -1;
    }
    const int64_t per_block = block_bytes(h.weighted, h.particles, h.particle_bytes);
    if (avail < per_block) {
        snprintf(msg, msg_len, "bytes %lld / %lld", (long long)avail, (long long)per_block);
        return -1;
    }
    if (!hist) {
        if (h.hist_cnt != 0) {
            snprintf(msg, msg_len, "hist_cnt 0x%08x / 0: record format %d has no history entries", (unsigned)h.hist_cnt, (int)w.record_format);
            return -1;
        }
        if ((int64_t)h.stride != (int64_t)w.particle_bytes) {
            snprintf(msg, msg_len, "record stride %u / %d", (unsigned)h.stride, (int)w.particle_bytes);
            return -1;
        }
        if (dst_stride) *dst_stride = w.particle_bytes;
        return 0;
    }
    for (int a = w.actions; a < 4; ++a)
        if ((h.hist_cnt >> (8 * a)) & 0xffu) {
            snprintf(msg, msg_len, "hist_cnt 0x%08x: entries of action %d, the context has %d actions", (unsigned)h.hist_cnt, a, (int)w.actions);
            return -1;
        }
    const int total = history_total(h.hist_cnt), src_room = (int)(h.particle_bytes / 4 - 2);
    if (w.actions > 4 || total > src_room) {
        snprintf(msg, msg_len, "hist_cnt 0x%08x: %d entries per record / room for %d in the block's own records", (unsigned)h.hist_cnt, total, src_room);
        return -1;
    }
    const int64_t stride = history_stride_bytes(h.particle_bytes, total, acc.compact != 0);
    if ((int64_t)h.stride != stride) {
        snprintf(msg, msg_len, "record stride %u / %lld for %d entries per record of %d bytes", (unsigned)h.stride, (long long)stride, total, (int)h.particle_bytes);
        return -1;
    }
    if (total > acc.hist_cap) {
        snprintf(msg, msg_len, "holds %d entries per record / room for %d", total, (int)acc.hist_cap);
        return -2;
    }
    if (dst_stride) *dst_stride = history_stride_bytes(w.particle_bytes, total, acc.compact != 0);
    return 0;
}

// The room rule of a resumed span (fba_run_bapomdp_span): a run that continues from this block through episodes [first, stop) must never
// hold more than an uninterrupted run of a context of `episodes` episodes of `horizon` steps could -- every bound fba_create derives from
// episodes * horizon (the entries a history record has room for, the uint16 increments of a packed record, the 15 bits a 16-byte tiger
// record keeps of one, the exactness of prior + j) then holds as it does there.  What the block holds already: the entries per record
// of a history format, head.updates of a packed one; fp32 counts (format 0) have no such bound.  A step makes one update at most.
// 0 = there is room; -1 = refused, with the block, both numbers and the span in msg.  Reads the 64 bytes of the header only.
inline int check_span_room(const void* block, int block_index, int32_t first, int32_t stop, int32_t episodes, int32_t horizon, char* msg, size_t msg_len)
{
    fba_snapshot_head h;
    memcpy(&h, block, sizeof h);
    if (h.record_format == 0) return 0;
    const bool hist     = h.record_format >= 5;
    const int64_t held  = hist ? (int64_t)history_total(h.hist_cnt) : (int64_t)h.updates;
    const int64_t more  = ((int64_t)stop - (int64_t)first) * (int64_t)horizon, room = (int64_t)episodes * (int64_t)horizon;
    if (held + more <= room) return 0;
    snprintf(msg, msg_len, "block %d holds %lld %s, episodes [%d, %d) of %d steps may add %lld: %lld / %lld (episodes * horizon) a run of this context holds",
             block_index, (long long)held, hist ? "history entries per record" : "counted updates", (int)first, (int)stop, (int)horizon, (long long)more,
             (long long)(held + more), (long long)room);
    return -1;
}

}  // namespace fba_snapshot
