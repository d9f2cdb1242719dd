// snapshot_format_check.cpp -- the host pass of fba_belief_import (fba_snapshot_format.h: check_head) fed good, truncated, zeroed and
// bit-flipped headers, as a stand-alone host program: tests/test_belief_snapshot_cpu.py builds it with the host compiler under
// -fsanitize=address,undefined and runs it as a child process.  Every block lives in a heap buffer of exactly the bytes it claims to
// have, so a read behind them is a report.  Exit status 0: every bad header was refused with a message and the good ones were taken.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "fba_snapshot_format.h"

namespace {

int failures = 0;

void expect(bool ok, const char* what, const std::string& detail = "")
{
    if (ok) return;
    ++failures;
    std::fprintf(stderr, "FAILED: %s %s\n", what, detail.c_str());
}

// check_head over a heap copy of exactly `avail` bytes of `block`
int check(const std::vector<unsigned char>& block, long long avail, const fba_snapshot::Accepts& acc, std::string& msg)
{
    unsigned char* exact = avail > 0 ? static_cast<unsigned char*>(std::malloc((size_t)avail)) : nullptr;
    if (avail > 0) std::memcpy(exact, block.data(), (size_t)avail);
    char buf[256] = "";
    const int rc = fba_snapshot::check_head(exact, avail, acc, buf, sizeof buf);
    msg = buf;
    std::free(exact);
    return rc;
}

fba_snapshot::Accepts context(int record_format, int weighted, int particles, int particle_bytes, int hist_cap)
{
    fba_snapshot::Accepts acc{};
    fba_snapshot_head& h = acc.want;
    h.magic = FBA_SNAPSHOT_MAGIC; h.version = FBA_SNAPSHOT_VERSION;
    h.record_format = (uint8_t)record_format; h.weighted = (uint8_t)weighted;
    h.model = FBA_MODEL_BA_FACTORED; h.domain = FBA_DOM_GRIDWORLD; h.actions = 4;
    h.size = 3; h.width = 0; h.height = 0;
    h.particles = particles; h.particle_bytes = particle_bytes; h.counts_len = 1234;
    h.states = 27; h.observations = 27;
    h.prior_hash = 0x0123456789abcdefull;
    acc.hist_cap = hist_cap;
    acc.compact  = 1;
    return acc;
}

std::vector<unsigned char> block_of(const fba_snapshot::Accepts& acc, uint32_t hist_cnt)
{
    fba_snapshot_head h = acc.want;
    h.hist_cnt = hist_cnt;
    h.stride   = (uint32_t)(h.record_format >= 5 ? fba_snapshot::history_stride_bytes(h.particle_bytes, fba_snapshot::history_total(hist_cnt), true)
                                                 : h.particle_bytes);
    std::vector<unsigned char> b((size_t)fba_snapshot::block_bytes(h.weighted, h.particles, h.particle_bytes), 0);
    h.checksum = fba_snapshot::checksum(b.data() + sizeof h, (b.size() - sizeof h) / 4);
    std::memcpy(b.data(), &h, sizeof h);
    return b;
}

}  // namespace

int main()
{
    static_assert(sizeof(fba_snapshot_head) == 64, "the header is 64 bytes");
    std::string msg;
    const fba_snapshot::Accepts hist = context(5, 1, 130, 144, 32), dense = context(0, 0, 7, 112, 0);
    const long long per = fba_snapshot::block_bytes(1, 130, 144);
    expect(per == 64 + 130 * 8 + 130 * 144, "block_bytes");

    // good headers at every stride are taken
    const uint32_t cnts[] = {0u, 0x00000e00u, 0x0000000fu, 0x1e000000u, 0x0a0a0a01u, 0x08080808u};
    const uint32_t strides[] = {64u, 64u, 128u, 128u, 144u, 144u};
    for (int k = 0; k < 6; ++k) {
        const std::vector<unsigned char> good = block_of(hist, cnts[k]);
        fba_snapshot_head h;
        std::memcpy(&h, good.data(), sizeof h);
        expect(h.stride == strides[k], "stride of a good header");
        expect(check(good, per, hist, msg) == 0, "a good header is taken:", msg);
    }
    expect(check(block_of(dense, 0), (long long)block_of(dense, 0).size(), dense, msg) == 0, "a good fp32 header is taken:", msg);

    const std::vector<unsigned char> good = block_of(hist, 0x00010203u);
    // truncated: every length short of a block, a few bytes of header included, and none at all
    for (long long avail : {0LL, 1LL, 3LL, 4LL, 31LL, 63LL, 64LL, 65LL, per / 2, per - 1}) {
        expect(check(good, avail, hist, msg) == -1, "a truncated block is refused");
        expect(msg.find("bytes") != std::string::npos, "... with a message that names the bytes:", msg);
    }
    {
        char buf[64];
        expect(fba_snapshot::check_head(nullptr, per, hist, buf, sizeof buf) == -1, "a null block is refused");
    }
    // zeroed: the whole header, and each field alone (a zero that a field may hold is skipped: hist_cnt 0 goes with the stride 64 only)
    {
        std::vector<unsigned char> z = good;
        std::memset(z.data(), 0, 64);
        expect(check(z, per, hist, msg) == -1 && msg.find("magic") != std::string::npos, "a zeroed header is refused by its magic:", msg);
    }
    struct Field { int at, len; const char* says; };
    const Field fields[] = {{0, 4, "magic"}, {4, 2, "layout version"}, {6, 1, "record format"}, {7, 1, "weighted"}, {8, 1, "model"}, {9, 1, "domain"},
                            {10, 2, "actions"}, {12, 2, "size"}, {20, 4, "particles"}, {24, 4, "particle bytes"}, {28, 4, "counts length"},
                            {32, 4, "states"}, {36, 4, "observations"}, {44, 4, "record stride"}, {48, 8, "prior hash"}};
    for (const Field& f : fields) {
        std::vector<unsigned char> z = good;
        std::memset(z.data() + f.at, 0, (size_t)f.len);
        expect(check(z, per, hist, msg) == -1 && msg.find(f.says) != std::string::npos, "a zeroed field is refused by name:", std::string(f.says) + " / " + msg);
    }
    // bit-flipped: every bit of the 56 bytes the host pass judges (the checksum is the device pass's), one at a time.  A flip in the
    // `updates` field or the reserved bits of no field is not a fingerprint change; everything else must be refused
    int refused = 0, taken = 0;
    for (int bit = 0; bit < 56 * 8; ++bit) {
        std::vector<unsigned char> f = good;
        f[(size_t)(bit / 8)] ^= (unsigned char)(1u << (bit % 8));
        const int rc = check(f, per, hist, msg);
        const bool free_field = bit / 8 == 18 || bit / 8 == 19;   // updates
        if (rc == 0) {
            ++taken;
            if (!free_field) {
                // a flip inside hist_cnt may give another legal split of the same stride class: legal by the format, judged by the device pass
                fba_snapshot_head h;
                std::memcpy(&h, f.data(), sizeof h);
                const int total = fba_snapshot::history_total(h.hist_cnt);
                expect(bit / 8 >= 40 && bit / 8 < 44 && total <= 32 && fba_snapshot::history_stride_bytes(144, total, true) == (long long)h.stride,
                       "a flipped fingerprint bit is refused, bit", std::to_string(bit));
            }
        } else {
            ++refused;
            expect(!msg.empty(), "a refusal has a message");
        }
    }
    expect(refused >= 52 * 8 - 32, "nearly every flipped bit is refused", std::to_string(refused) + " refused, " + std::to_string(taken) + " taken");
    // hist_cnt against the record: too many entries, entries of an action the context lacks, an fp32 block with entries
    {
        std::vector<unsigned char> b = block_of(hist, 0x10101010u);
        expect(check(b, per, hist, msg) == -1 && msg.find("room for 32") != std::string::npos, "64 entries in a record of 32:", msg);
        fba_snapshot::Accepts three = hist;
        three.want.actions = 3;
        b = block_of(three, 0x01000000u);
        expect(check(b, per, three, msg) == -1 && msg.find("action 3") != std::string::npos, "entries of action 3 of 3:", msg);
        b = block_of(dense, 0);
        b[40] = 1;
        expect(check(b, (long long)b.size(), dense, msg) == -1 && msg.find("hist_cnt") != std::string::npos, "an fp32 block with entries:", msg);
    }
    // the checksum formula on the host: the order of the words' terms cannot matter, and one changed word changes it
    {
        uint32_t w[5] = {7u, 0u, 0xffffffffu, 12345u, 1u};
        uint64_t by_hand = 0;
        for (int i = 4; i >= 0; --i) by_hand += (uint64_t)w[i] * ((uint64_t)(i + 1) * FBA_SNAPSHOT_CHECK_MUL);
        expect(fba_snapshot::checksum(w, 5) == by_hand, "checksum against the formula");
        w[3] ^= 0x100u;
        expect(fba_snapshot::checksum(w, 5) != by_hand, "checksum of a changed word");
        expect(fba_snapshot::checksum(reinterpret_cast<unsigned char*>(w) + 4, 3) != 0, "checksum of an unaligned payload");
    }
    if (failures) {
        std::fprintf(stderr, "%d checks failed\n", failures);
        return 1;
    }
    std::printf("snapshot_format_check: ok (%d flipped bits refused, %d taken)\n", refused, taken);
    return 0;
}
