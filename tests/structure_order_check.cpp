// structure_order_check.cpp -- the host-callable helpers of fba_belief_structures (fba_structures.h): the hash that keys the table of
// distinct structures, equality of word lists and the order of the top list, as a stand-alone host program.
// tests/test_structures_abi.py builds it with the host compiler under -fsanitize=address,undefined and runs it as a child process.
// Exit status 0: every check held.
#include <algorithm>
#include <cstdio>
#include <cstdint>
#include <set>
#include <vector>

#include "fba_structures.h"

namespace {

int failures = 0;
void expect(bool ok, const char* what)
{
    if (ok) return;
    ++failures;
    std::fprintf(stderr, "FAILED: %s\n", what);
}

using List = std::vector<uint32_t>;
struct Words {
    const List* l;
    uint32_t operator()(int m) const { return (*l)[(size_t)m]; }
};
uint64_t hash_of(const List& l, uint64_t keep = ~0ull) { return fba::struct_hash(Words{&l}, (int)l.size(), keep); }

// the table of structures_kernel, one particle after the other: open addressing from the hash, an entry of the same hash is the
// particle's only where the representative's words are the same
struct Table {
    std::vector<uint64_t> hash;
    std::vector<int> rep;
    std::vector<double> mass;
    explicit Table(size_t n) : hash(n, fba::STRUCT_HASH_FREE), rep(n, -1), mass(n, 0.0) {}
    bool add(const std::vector<List>& all, int i, double w, uint64_t keep)
    {
        const uint64_t h = hash_of(all[(size_t)i], keep);
        size_t pos = (size_t)(h >> 20) % hash.size();
        for (size_t probe = 0; probe < hash.size(); ++probe, pos = (pos + 1) % hash.size()) {
            if (hash[pos] == fba::STRUCT_HASH_FREE) { hash[pos] = h; rep[pos] = i; mass[pos] = w; return true; }
            if (hash[pos] == h && fba::struct_compare(Words{&all[(size_t)i]}, Words{&all[(size_t)rep[pos]]}, (int)all[(size_t)i].size()) == 0) { mass[pos] += w; return true; }
        }
        return false;
    }
    int distinct() const { return (int)std::count_if(hash.begin(), hash.end(), [](uint64_t h) { return h != fba::STRUCT_HASH_FREE; }); }
};

}  // namespace

int main()
{
    // the hash: never the mark of a free entry, whatever bits are kept; different for lists that differ in one word or in length
    std::set<uint64_t> seen;
    int lists = 0;
    for (uint32_t n = 1; n <= 20; ++n)
        for (uint32_t v = 0; v < 256; ++v) {
            List l(n, 3u);
            l[n - 1] = v;
            const uint64_t h = hash_of(l);
            expect(h != fba::STRUCT_HASH_FREE, "a hash is never the free mark");
            expect(hash_of(l, 0) == 1ull, "no bit kept: every list hashes to 1");
            expect((hash_of(l, 0xff) & ~0xffull) == 0 && hash_of(l, 0xff) != fba::STRUCT_HASH_FREE, "kept bits only");
            seen.insert(h);
            ++lists;
        }
    expect((int)seen.size() == lists, "5120 lists that differ in the last word or in length: 5120 hashes");

    // compare and order: word 0 is the most significant; the larger mass first, among equal masses the smaller list
    const List a{3, 7, 1}, b{3, 7, 2}, c{4, 0, 0}, d{3, 7, 1};
    expect(fba::struct_compare(Words{&a}, Words{&b}, 3) < 0, "{3,7,1} < {3,7,2}");
    expect(fba::struct_compare(Words{&b}, Words{&a}, 3) > 0, "{3,7,2} > {3,7,1}");
    expect(fba::struct_compare(Words{&b}, Words{&c}, 3) < 0, "{3,7,2} < {4,0,0}");
    expect(fba::struct_compare(Words{&a}, Words{&d}, 3) == 0, "{3,7,1} == {3,7,1}");
    expect(fba::struct_compare(Words{&a}, Words{&b}, 2) == 0, "the first two words are the same");
    expect(fba::struct_before(2.0, Words{&c}, 1.0, Words{&a}, 3), "the larger mass first");
    expect(!fba::struct_before(1.0, Words{&a}, 2.0, Words{&c}, 3), "the smaller mass not first");
    expect(fba::struct_before(1.0, Words{&a}, 1.0, Words{&b}, 3), "equal masses: the smaller list first");
    expect(!fba::struct_before(1.0, Words{&b}, 1.0, Words{&a}, 3), "equal masses: the larger list not first");
    expect(!fba::struct_before(1.0, Words{&a}, 1.0, Words{&d}, 3), "an entry is not before itself");

    // equal hashes: two structures that differ only in the last word are two entries, with every hash the same and with real hashes
    for (uint64_t keep : {0ull, 0x3ull, ~0ull}) {
        std::vector<List> all;
        for (int i = 0; i < 40; ++i) {
            List l(5, 7u);
            l[4] = (uint32_t)(i % 10);
            all.push_back(l);
        }
        Table t(16);
        bool placed = true;
        for (int i = 0; i < 40; ++i) placed = t.add(all, i, 1.0, keep) && placed;
        expect(placed, "ten structures find a place among sixteen entries");
        expect(t.distinct() == 10, "ten structures that differ in the last word: ten entries");
        double total = 0.0;
        for (size_t k = 0; k < t.mass.size(); ++k) {
            total += t.mass[k];
            expect(t.hash[k] == fba::STRUCT_HASH_FREE || t.mass[k] == 4.0, "four particles per structure");
        }
        expect(total == 40.0, "every particle is counted once");
        // a full table holds exactly its size; one more structure finds no place
        Table full(10);
        for (int i = 0; i < 40; ++i) expect(full.add(all, i, 1.0, keep), "exactly as many structures as entries: all placed");
        all.push_back(List(5, 1u));
        expect(!full.add(all, 40, 1.0, keep), "one structure more than entries: no place");
    }

    if (failures) return 1;
    std::printf("structure_order_check: ok\n");
    return 0;
}
