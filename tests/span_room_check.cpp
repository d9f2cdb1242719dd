// span_room_check.cpp -- the room rule of a resumed span (fba_snapshot_format.h: check_span_room) at its edges, as a stand-alone host
// program: tests/test_belief_resume_cpu.py builds it with the host compiler under -fsanitize=address,undefined and runs it as a child
// process.  Every header lives in a heap buffer of exactly its 64 bytes, so a read behind them is a report.  Exit status 0: every span
// that fits was taken, every one that does not was refused with the block, both numbers and the span in the message.
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

// check_span_room over a heap copy of exactly the header
int room(int record_format, uint32_t hist_cnt, unsigned updates, int block, int first, int stop, int episodes, int horizon, std::string& msg)
{
    fba_snapshot_head h{};
    h.magic = FBA_SNAPSHOT_MAGIC; h.version = FBA_SNAPSHOT_VERSION;
    h.record_format = (uint8_t)record_format;
    h.hist_cnt = hist_cnt; h.updates = (uint16_t)updates;
    unsigned char* exact = static_cast<unsigned char*>(std::malloc(sizeof h));
    std::memcpy(exact, &h, sizeof h);
    char buf[320] = "";
    const int rc = fba_snapshot::check_span_room(exact, block, first, stop, episodes, horizon, buf, sizeof buf);
    msg = buf;
    std::free(exact);
    return rc;
}

bool has(const std::string& msg, const char* part) { return msg.find(part) != std::string::npos; }

}  // namespace

int main()
{
    std::string msg;
    // history records (formats 5..7): the entries per record, summed over the actions, 8 bits each
    const uint32_t cnt16 = 5u | (4u << 8) | (4u << 16) | (3u << 24);   // 16 entries
    expect(room(5, cnt16, 0, 0, 2, 5, 5, 8, msg) == 0 && msg.empty(), "16 entries + 3 episodes of 8 = 40 of 40: taken", msg);
    expect(room(5, cnt16 + 1u, 0, 3, 2, 5, 5, 8, msg) == -1, "17 entries + 24 = 41 of 40: refused");
    expect(has(msg, "block 3 ") && has(msg, "17 history entries per record") && has(msg, "[2, 5)") && has(msg, "41 / 40"), "the message names block, numbers and span", msg);
    expect(room(6, cnt16, 0, 1, 1, 5, 5, 8, msg) == -1 && has(msg, "block 1 ") && has(msg, "may add 32") && has(msg, "48 / 40"), "16 + 32 of 40: refused", msg);
    expect(room(7, 0, 0, 0, 0, 5, 5, 8, msg) == 0, "an empty record and the whole experiment: taken", msg);
    expect(room(7, 0xffffffffu, 0, 0, 4, 5, 5, 8, msg) == -1 && has(msg, "1020 history entries"), "255 entries of every action: refused", msg);
    expect(room(5, cnt16, 65535, 0, 2, 5, 5, 8, msg) == 0, "head.updates of a history block is not its measure", msg);
    // packed records (formats 1..4): head.updates
    expect(room(1, 0, 16, 0, 2, 5, 5, 8, msg) == 0, "16 updates + 24 = 40 of 40: taken", msg);
    expect(room(1, 0, 17, 6, 2, 5, 5, 8, msg) == -1 && has(msg, "block 6 ") && has(msg, "17 counted updates") && has(msg, "41 / 40"), "17 updates + 24: refused", msg);
    expect(room(4, 0, 65535, 0, 0, 1, 65535, 1, msg) == -1 && has(msg, "65536 / 65535"), "the uint16 bound itself", msg);
    expect(room(3, 0, 65534, 0, 0, 1, 65535, 1, msg) == 0, "65534 + 1 of 65535: taken", msg);
    expect(room(2, 0, 0, 0, 0, 65535, 65535, 255, msg) == 0, "the largest experiment a context takes, from the prior's own block", msg);
    expect(room(2, 0, 1, 0, 0, 65535, 65535, 255, msg) == -1 && has(msg, "16711426 / 16711425"), "... and one update more: no overflow in the sum", msg);
    // fp32 counts (format 0): no such bound
    expect(room(0, 0, 65535, 0, 0, 5, 5, 8, msg) == 0 && msg.empty(), "fp32 counts: always room", msg);
    // a short message buffer is respected
    {
        fba_snapshot_head h{};
        h.record_format = 1; h.updates = 40;
        char tiny[8];
        expect(fba_snapshot::check_span_room(&h, 0, 1, 5, 5, 8, tiny, sizeof tiny) == -1 && std::strlen(tiny) < sizeof tiny, "a message buffer of 8 bytes");
    }
    if (failures) {
        std::fprintf(stderr, "span_room_check: %d failures\n", failures);
        return 1;
    }
    std::puts("span_room_check: ok");
    return 0;
}
