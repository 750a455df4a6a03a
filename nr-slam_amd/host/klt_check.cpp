// Stand-alone check of the host half of the tracker's template stores (csrc/nrs_klt_host.hpp) under AddressSanitizer + UBSan:
// `make klt_check` (builds and runs it).  No HIP, no library: hand-made lists, every array exactly as long as the interface says.
#include <cstdio>
#include <cstring>
#include <vector>
#include "../csrc/nrs_klt_host.hpp"

using namespace nrs;

static int fails = 0;
#define CHECK(cond) do { if (!(cond)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++fails; } } while (0)

int main() {
    char msg[256];
    int kmax = 0;
    // ---- what an entry holds: 441 i16, 441 (i16, i16), 2 f32 and 1 byte per level; 8 bytes of xy or 1 "has" byte per entry
    CHECK(KA == 441);
    CHECK(klt_entry_bytes(0, 1) == 882 && klt_entry_bytes(1, 1) == 1764 && klt_entry_bytes(2, 1) == 8 && klt_entry_bytes(3, 1) == 1);
    CHECK(klt_entry_bytes(0, 5) == 4410 && klt_entry_bytes(1, 5) == 8820 && klt_entry_bytes(2, 5) == 40 && klt_entry_bytes(3, 5) == 5);
    CHECK(KLT_XY_BYTES == 2 * sizeof(float) && KLT_HAS_BYTES == 1);
    {
        size_t per_level = 0;
        for (int a = 0; a < KLT_ARRAYS; ++a) per_level += klt_entry_bytes(a, 1);
        CHECK(per_level == 6u * KA + 9u);                          // ("KA x levels x 6 bytes per key" and the means and the valid byte)
    }
    // ---- the growth rule: max(want + want / 2, 256)
    CHECK(klt_grow_capacity(0) == 256);
    CHECK(klt_grow_capacity(1) == 256);
    CHECK(klt_grow_capacity(170) == 256 && klt_grow_capacity(171) == 256 && klt_grow_capacity(172) == 258);
    CHECK(klt_grow_capacity(255) == 382);
    CHECK(klt_grow_capacity(256) == 384);
    CHECK(klt_grow_capacity(257) == 385);
    CHECK(klt_grow_capacity(350) == 525 && klt_grow_capacity(1001) == 1501);
    CHECK(klt_grow_capacity(NRS_KLT_ARCHIVE_MAX_KEY) == NRS_KLT_ARCHIVE_MAX_KEY + NRS_KLT_ARCHIVE_MAX_KEY / 2);
    // ---- the checks, in their order
    const int n_stored = 6;
    {
        const std::vector<int32_t> slots = {3, 0, 5}, keys = {900, 2, 57};
        CHECK(klt_archive_check(3, slots.data(), keys.data(), true, n_stored, &kmax, msg, sizeof msg) == 0 && kmax == 900);
        CHECK(klt_archive_check(-1, slots.data(), keys.data(), true, n_stored, &kmax, msg, sizeof msg) == -1 && strstr(msg, "bad argument"));
        CHECK(klt_archive_check(3, nullptr, keys.data(), true, n_stored, &kmax, msg, sizeof msg) == -1 && strstr(msg, "bad argument"));
        CHECK(klt_archive_check(3, slots.data(), nullptr, true, n_stored, &kmax, msg, sizeof msg) == -1 && strstr(msg, "bad argument"));
        CHECK(klt_archive_check(3, slots.data(), keys.data(), false, 0, &kmax, msg, sizeof msg) == -2 && strstr(msg, "no tracker state"));
        CHECK(klt_archive_check(3, nullptr, nullptr, false, 0, &kmax, msg, sizeof msg) == -1);     // (the lists come before the state)
    }
    // n = 0: a valid call that reads no list and asks for no state
    CHECK(klt_archive_check(0, nullptr, nullptr, false, 0, &kmax, msg, sizeof msg) == 0 && kmax == -1);
    {
        std::vector<int> us = {7}, uk = {7};
        klt_archive_last_stands(0, nullptr, nullptr, -1, us, uk);
        CHECK(us.empty() && uk.empty());
    }
    // a slot at n, and below zero
    {
        const std::vector<int32_t> slots = {0, n_stored}, keys = {1, 2};
        CHECK(klt_archive_check(2, slots.data(), keys.data(), true, n_stored, &kmax, msg, sizeof msg) == -1 && strstr(msg, "slot 6 out of range"));
        const std::vector<int32_t> neg = {0, -1};
        CHECK(klt_archive_check(2, neg.data(), keys.data(), true, n_stored, &kmax, msg, sizeof msg) == -1 && strstr(msg, "slot -1 out of range"));
        const std::vector<int32_t> top = {0, n_stored - 1};
        CHECK(klt_archive_check(2, top.data(), keys.data(), true, n_stored, &kmax, msg, sizeof msg) == 0 && kmax == 2);
        CHECK(klt_archive_check(1, top.data(), keys.data(), true, 0, &kmax, msg, sizeof msg) == -1 && strstr(msg, "slot 0 out of range"));     // (a tracker that holds nothing)
    }
    // a key at the limit - 1 and one at the limit
    {
        const std::vector<int32_t> slots = {1, 2};
        const std::vector<int32_t> in = {NRS_KLT_ARCHIVE_MAX_KEY - 1, 0};
        CHECK(klt_archive_check(2, slots.data(), in.data(), true, n_stored, &kmax, msg, sizeof msg) == 0 && kmax == NRS_KLT_ARCHIVE_MAX_KEY - 1);
        std::vector<int> us, uk;
        klt_archive_last_stands(2, slots.data(), in.data(), kmax, us, uk);
        CHECK(us == std::vector<int>({1, 2}) && uk == std::vector<int>({NRS_KLT_ARCHIVE_MAX_KEY - 1, 0}));
        const std::vector<int32_t> at = {0, NRS_KLT_ARCHIVE_MAX_KEY};
        CHECK(klt_archive_check(2, slots.data(), at.data(), true, n_stored, &kmax, msg, sizeof msg) == -1);
        CHECK(strstr(msg, "key 1048576 out of range") && strstr(msg, "keys below 1048576"));
        const std::vector<int32_t> neg = {-1, 0};
        CHECK(klt_archive_check(2, slots.data(), neg.data(), true, n_stored, &kmax, msg, sizeof msg) == -1 && strstr(msg, "key -1 out of range"));
    }
    // ---- repeated keys: the last occurrence stands, the survivors keep their order
    {
        const std::vector<int32_t> slots = {3, 0, 5, 4, 1, 2}, keys = {900, 2, 57, 900, 2, 2};
        CHECK(klt_archive_check(6, slots.data(), keys.data(), true, n_stored, &kmax, msg, sizeof msg) == 0 && kmax == 900);
        std::vector<int> us, uk;
        klt_archive_last_stands(6, slots.data(), keys.data(), kmax, us, uk);
        CHECK(us == std::vector<int>({5, 4, 2}) && uk == std::vector<int>({57, 900, 2}));
        const std::vector<int32_t> same_key(4, 0), four = {0, 1, 2, 3};          // every entry under key 0 (kmax 0: a one-entry table)
        CHECK(klt_archive_check(4, four.data(), same_key.data(), true, n_stored, &kmax, msg, sizeof msg) == 0 && kmax == 0);
        klt_archive_last_stands(4, four.data(), same_key.data(), kmax, us, uk);
        CHECK(us == std::vector<int>({3}) && uk == std::vector<int>({0}));
    }
    printf(fails ? "klt_check: %d check(s) FAILED\n" : "klt_check OK\n", fails);
    return fails ? 1 : 0;
}
