// convert_head_check.cpp -- the host pass of fba_belief_convert (fba_snapshot_format.h: check_convert_head) as a stand-alone host program:
// tests/test_belief_convert_cpu.py builds it with the host compiler under -fsanitize=address,undefined and runs it as a child process.
// Every header lives in a heap buffer of exactly its 64 bytes, so a read behind them is a report.  Exit status 0: every fingerprint field
// was refused in turn with both values in the message, room and stride of a block were judged against the block's own room, and the
// destination stride came out as the context stores records of that many entries.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "fba_snapshot_format.h"

namespace {

int failures = 0;

void expect(bool ok, const char* what, const std::string& detail = "")
{
    if (ok) return;
    ++failures;
    std::fprintf(stderr, "FAILED: %s %s\n", what, detail.c_str());
}
bool has(const std::string& msg, const char* part) { return msg.find(part) != std::string::npos; }

// a gridworld history context (format 5, weighted) of 130 particles whose records have room for `cap` entries
fba_snapshot::Accepts context(int cap, bool compact = true, int format = 5)
{
    fba_snapshot::Accepts acc{};
    fba_snapshot_head& h = acc.want;
    h.magic = FBA_SNAPSHOT_MAGIC; h.version = FBA_SNAPSHOT_VERSION;
    h.record_format = (uint8_t)format; h.weighted = 1; h.model = 2; h.domain = 4; h.actions = 4;
    h.size = 3; h.width = 0; h.height = 0;
    h.particles = 130; h.particle_bytes = format >= 5 ? 4 * ((2 + cap + 3) & ~3) : 64; h.counts_len = 1000; h.states = 36; h.observations = 36;
    h.prior_hash = 0x0123456789abcdefull;
    acc.hist_cap = format >= 5 ? cap : 0;
    acc.compact  = compact ? 1 : 0;
    return acc;
}
// a block header of a context like `acc` but for its particles and the room of its records, holding `total` entries per record
fba_snapshot_head block_of(const fba_snapshot::Accepts& acc, int particles, int particle_bytes, int total, bool compact = true)
{
    fba_snapshot_head h = acc.want;
    h.particles = particles; h.particle_bytes = particle_bytes;
    const int per = total / 4, rest = total - 4 * per;   // spread over the four actions
    h.hist_cnt = (uint32_t)(per + rest) | ((uint32_t)per << 8) | ((uint32_t)per << 16) | ((uint32_t)per << 24);
    h.stride = (uint32_t)(acc.want.record_format >= 5 ? fba_snapshot::history_stride_bytes(particle_bytes, total, compact) : particle_bytes);
    return h;
}
// check_convert_head over a heap copy of exactly the header; avail says how much the caller claims is readable
int judge(const fba_snapshot_head& h, const fba_snapshot::Accepts& acc, int src_particles, int src_bytes, std::string& msg, int64_t* stride = nullptr, int64_t avail = -1)
{
    unsigned char* exact = static_cast<unsigned char*>(std::malloc(sizeof h));
    std::memcpy(exact, &h, sizeof h);
    char buf[256] = "";
    if (avail < 0) avail = fba_snapshot::block_bytes(h.weighted, h.particles, h.particle_bytes);
    const int rc = fba_snapshot::check_convert_head(exact, avail, acc, src_particles, src_bytes, buf, sizeof buf, stride);
    msg = buf;
    std::free(exact);
    return rc;
}

}  // namespace

int main()
{
    std::string msg;
    const fba_snapshot::Accepts dst = context(40);   // 5 episodes of 8 steps: records of 176 bytes
    expect(dst.want.particle_bytes == 176, "a 40-entry record has 176 bytes");
    // ---- what may differ: particles, and the room of a history record
    {
        int64_t stride = -1;
        expect(judge(block_of(dst, 130, 176, 20), dst, 130, 176, msg, &stride) == 0 && stride == 128 && msg.empty(), "the context's own block", msg);
        expect(judge(block_of(dst, 300, 176, 20), dst, 300, 176, msg, &stride) == 0 && stride == 128, "another particle count", msg);
        expect(judge(block_of(dst, 37, 80, 15), dst, 37, 80, msg, &stride) == 0 && stride == 128, "another particle count and another room", msg);
    }
    // ---- every other fingerprint field, refused in turn with both values
    struct Flip { const char* name; void (*set)(fba_snapshot_head&); const char* says; };
    const Flip flips[] = {
        {"magic", [](fba_snapshot_head& h) { h.magic ^= 1u; }, "magic 0x"},
        {"version", [](fba_snapshot_head& h) { h.version = 2; }, "layout version 2 / 1"},
        {"record_format", [](fba_snapshot_head& h) { h.record_format = 6; }, "record format 6 in the block, 5 in this context"},
        {"weighted", [](fba_snapshot_head& h) { h.weighted = 0; }, "weighted 0 in the block, 1 in this context"},
        {"model", [](fba_snapshot_head& h) { h.model = 1; }, "model 1 in the block, 2 in this context"},
        {"domain", [](fba_snapshot_head& h) { h.domain = 5; }, "domain 5 in the block, 4 in this context"},
        {"size", [](fba_snapshot_head& h) { h.size = 4; }, "size 4 in the block, 3 in this context"},
        {"width", [](fba_snapshot_head& h) { h.width = 5; }, "width 5 in the block, 0 in this context"},
        {"height", [](fba_snapshot_head& h) { h.height = 7; }, "height 7 in the block, 0 in this context"},
        {"counts_len", [](fba_snapshot_head& h) { h.counts_len = 999; }, "counts length 999 in the block, 1000 in this context"},
        {"states", [](fba_snapshot_head& h) { h.states = 35; }, "states 35 in the block, 36 in this context"},
        {"actions", [](fba_snapshot_head& h) { h.actions = 3; }, "actions 3 in the block, 4 in this context"},
        {"observations", [](fba_snapshot_head& h) { h.observations = 37; }, "observations 37 in the block, 36 in this context"},
        {"prior_hash", [](fba_snapshot_head& h) { h.prior_hash ^= 1ull << 40; }, "prior hash 0123446789abcdef in the block, 0123456789abcdef in this context"},
    };
    for (const Flip& f : flips) {
        fba_snapshot_head h = block_of(dst, 300, 80, 10);
        f.set(h);
        expect(judge(h, dst, 300, 80, msg) == -1 && has(msg, f.says), f.name, msg);
    }
    // ... and the two that may differ from the context must still be those of the call's first block
    expect(judge(block_of(dst, 300, 80, 10), dst, 130, 80, msg) == -1 && has(msg, "particles 300 in the block, 130 in the first block"), "particles of another block", msg);
    expect(judge(block_of(dst, 300, 80, 10), dst, 300, 144, msg) == -1 && has(msg, "particle bytes 80 in the block, 144 in the first block"), "room of another block", msg);
    expect(judge(block_of(dst, 0, 80, 0), dst, 0, 80, msg) == -1 && has(msg, "particles 0"), "no particles", msg);
    expect(judge(block_of(dst, -5, 80, 0), dst, -5, 80, msg, nullptr, 64) == -1 && has(msg, "particles -5"), "a negative particle count", msg);
    expect(judge(block_of(dst, 130, 4, 0), dst, 130, 4, msg) == -1 && has(msg, "particle bytes 4"), "a history record without its two words", msg);
    expect(judge(block_of(dst, 130, 82, 0), dst, 130, 82, msg) == -1 && has(msg, "particle bytes 82"), "a record of half a word", msg);
    // the formats without history entries: particle_bytes is part of what must match
    {
        const fba_snapshot::Accepts packed = context(0, true, 1);
        int64_t stride = -1;
        expect(judge(block_of(packed, 37, 64, 0), packed, 37, 64, msg, &stride) == 0 && stride == 64, "packed records, another particle count", msg);
        expect(judge(block_of(packed, 37, 128, 0), packed, 37, 128, msg) == -1 && has(msg, "particle bytes 128 in the block, 64 in this context"), "packed records of another size", msg);
        fba_snapshot_head h = block_of(packed, 37, 64, 0);
        h.hist_cnt = 1;
        expect(judge(h, packed, 37, 64, msg) == -1 && has(msg, "has no history entries"), "entries in a format without them", msg);
        h = block_of(packed, 37, 64, 0);
        h.stride = 128;
        expect(judge(h, packed, 37, 64, msg) == -1 && has(msg, "record stride 128 / 64"), "a stride other than the record", msg);
    }
    // ---- bytes: a header cut short, a block cut short; nothing behind the 64 bytes is read
    expect(judge(block_of(dst, 130, 80, 3), dst, 130, 80, msg, nullptr, 63) == -1 && has(msg, "bytes 63 / 64"), "63 bytes", msg);
    expect(judge(block_of(dst, 130, 80, 3), dst, 130, 80, msg, nullptr, 64 + 130 * 88 - 1) == -1 && has(msg, "bytes 11503 / 11504"), "one byte short of a block", msg);
    {
        char buf[64];
        expect(fba_snapshot::check_convert_head(nullptr, 1 << 20, dst, 1, 80, buf, sizeof buf) == -1, "a null block");
    }
    // ---- room and stride, judged against the SOURCE's room
    {
        // an 80-byte record has room for 18 entries (a context of 2 x 8 steps uses 16 of them)
        expect(judge(block_of(dst, 130, 80, 18), dst, 130, 80, msg) == 0, "18 entries in 80 bytes", msg);
        fba_snapshot_head h = block_of(dst, 130, 80, 18);
        h.hist_cnt += 1;
        expect(judge(h, dst, 130, 80, msg) == -1 && has(msg, "19 entries per record / room for 18 in the block's own records"), "19 entries in 80 bytes", msg);
        // 15 entries: 68 bytes, whole 80-byte records -- not the 128 the destination would store them at
        h = block_of(dst, 130, 80, 15);
        expect(h.stride == 80, "15 entries of an 80-byte record stand at 80");
        h.stride = 128;
        expect(judge(h, dst, 130, 80, msg) == -1 && has(msg, "record stride 128 / 80 for 15 entries per record of 80 bytes"), "the destination's stride in a source block", msg);
        h = block_of(dst, 130, 144, 31);
        expect(h.stride == 144 && judge(h, dst, 130, 144, msg) == 0, "31 entries of a 144-byte record stand at 144", msg);
        h.stride = 176;
        expect(judge(h, dst, 130, 144, msg) == -1 && has(msg, "record stride 176 / 144"), "... not at 176", msg);
        h = block_of(dst, 130, 144, 14);
        h.stride = 144;
        expect(judge(h, dst, 130, 144, msg) == -1 && has(msg, "record stride 144 / 64"), "short histories stand at 64 in a compact context", msg);
        const fba_snapshot::Accepts whole = context(40, false);
        expect(judge(h, whole, 130, 144, msg) == 0, "... and whole where the context stores every record whole", msg);
        h = block_of(dst, 130, 80, 4);
        h.hist_cnt = 1u << 24;
        fba_snapshot::Accepts three = dst;
        three.want.actions = 3;
        h.actions = 3;
        expect(judge(h, three, 130, 80, msg) == -1 && has(msg, "entries of action 3, the context has 3 actions"), "entries of an action the context lacks", msg);
    }
    // ---- the destination's room and stride
    {
        const fba_snapshot::Accepts small = context(16);   // 2 episodes of 8 steps
        expect(small.want.particle_bytes == 80, "a 16-entry record has 80 bytes");
        expect(judge(block_of(small, 130, 176, 16), small, 130, 176, msg) == 0, "16 entries into room for 16", msg);
        expect(judge(block_of(small, 130, 176, 17), small, 130, 176, msg) == -2 && msg == "holds 17 entries per record / room for 16", "17 entries into room for 16", msg);
        expect(judge(block_of(small, 130, 176, 32), small, 130, 176, msg) == -2 && msg == "holds 32 entries per record / room for 16", "32 entries into room for 16", msg);
        const int totals[] = {0, 14, 15, 30, 31};
        const int rooms[] = {80, 144, 176};
        for (int bytes : rooms) {
            const fba_snapshot::Accepts acc = context(bytes / 4 - 4), full = context(bytes / 4 - 4, false);
            expect(acc.want.particle_bytes == bytes, "the destination's record size");
            for (int total : totals) {
                int64_t stride = -1, expected = total <= 14 ? 64 : (total <= 30 && bytes > 128 ? 128 : bytes);
                const fba_snapshot_head h = block_of(acc, 300, 176, total);
                const int rc = judge(h, acc, 300, 176, msg, &stride);
                if (total > acc.hist_cap) {
                    expect(rc == -2, "more entries than the destination has room for", msg);
                    continue;
                }
                expect(rc == 0 && stride == expected, "the destination stride", std::to_string(bytes) + " bytes, " + std::to_string(total) + " entries: " + std::to_string(stride) + " " + msg);
                stride = -1;
                expect(judge(block_of(full, 300, 176, total, false), full, 300, 176, msg, &stride) == 0 && stride == bytes, "... of a context that stores records whole", msg);
            }
        }
    }
    // a short message buffer is respected
    {
        fba_snapshot_head h = block_of(dst, 130, 80, 3);
        h.states = 1;
        char tiny[8];
        expect(fba_snapshot::check_convert_head(&h, 1 << 20, dst, 130, 80, tiny, sizeof tiny) == -1 && std::strlen(tiny) < sizeof tiny, "a message buffer of 8 bytes");
    }
    if (failures) {
        std::fprintf(stderr, "convert_head_check: %d failures\n", failures);
        return 1;
    }
    std::puts("convert_head_check: ok");
    return 0;
}
