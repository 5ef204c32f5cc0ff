// The 8-byte schedule word's encode / decode (nfgpu_device.hpp: sc_encode, sc_decode, sc_fits) on the
// host: every field at its bounds and one past them.  A record that sc_encode takes must decode to
// itself bit for bit; one it refuses (returns 0) must be one of the documented wide cases.
// Built with the host's address / undefined-behaviour sanitizers (tests/test_sched_compact.py).
#include <cstdio>
#include <cstdlib>

#include "../../noahgameframe_amd/csrc/nfgpu_device.hpp"

using namespace nfgpu;

static int fails = 0;
#define EXPECT(c)                                          \
    do {                                                   \
        if (!(c)) {                                        \
            printf("FAIL %s:%d  %s\n", __FILE__, __LINE__, #c); \
            fails++;                                       \
        }                                                  \
    } while (0)

static bool same(const SchedHot& a, const SchedHot& b) {
    return a.next == b.next && a.remain == b.remain && a.state == b.state;
}

// expect: whether the record is compact under (epoch, step)
static void check(int64_t epoch, int32_t step, int64_t next, int32_t remain, uint32_t flags, int64_t rec_step, bool expect) {
    SchedHot h;
    h.next = next;
    h.remain = remain;
    h.state = flags | st_pack_step(rec_step);
    const uint64_t w = sc_encode(h, epoch, step, true);
    EXPECT((w != 0) == expect);
    if (w) {
        EXPECT(!(w & kScWide) && (w & kStPresent));
        EXPECT(same(sc_decode(w, epoch, step), h));
        EXPECT(sc_off(w) == next - epoch && sc_remain(w) == remain);
    } else if (h.state & kStPresent) {
        const uint64_t ww = sc_wide_word(h.state);
        EXPECT((ww & kScWide) && (ww & kStPresent) && ((ww & kStForever) != 0) == ((h.state & kStForever) != 0));
    }
    EXPECT(sc_encode(h, epoch, step, false) == 0);  // a kind without a common step has no compact records
}

int main() {
    const int64_t top = 1ll << kScNextBits;                 // first offset past the field
    const int32_t rlo = -(1 << (kScRemBits - 1)), rhi = (1 << (kScRemBits - 1)) - 1;
    const int64_t epochs[] = {0, 1700000000000ll - kScEpochBack, -(1ll << 40), (1ll << 62)};
    const int32_t steps[] = {100, 1, -50, (1 << 27) - 1, -(1 << 27), 0};
    for (int64_t epoch : epochs)
        for (int32_t step : steps) {
            // next: both ends of the window and one past each
            for (uint32_t fl : {kStPresent, kStPresent | kStFired}) {
                check(epoch, step, epoch, 5, fl, step, true);
                check(epoch, step, epoch - 1, 5, fl, step, false);
                check(epoch, step, epoch + top - 1, 5, fl, step, true);
                check(epoch, step, epoch + top, 5, fl, step, false);
                check(epoch, step, epoch + kScEpochBack, 0, fl, step, true);   // a zero count: present, never fires
                // remain of a counted schedule: both ends and one past the top
                check(epoch, step, epoch + 7, rhi, fl, step, true);
                check(epoch, step, epoch + 7, rhi + 1, fl, step, false);
                check(epoch, step, epoch + 7, INT32_MAX, fl, step, false);
            }
            for (uint32_t fl : {kStPresent | kStForever, kStPresent | kStForever | kStFired}) {
                // remain of a forever schedule: -1 down to the field's lower bound, one past it, and wrapped
                check(epoch, step, epoch + 7, -1, fl, step, true);
                check(epoch, step, epoch + 7, rlo, fl, step, true);
                check(epoch, step, epoch + 7, rlo - 1, fl, step, false);
                check(epoch, step, epoch + 7, INT32_MIN, fl, step, false);
                check(epoch, step, epoch + 7, 0, fl, step, false);          // wrapped through INT32_MIN
                check(epoch, step, epoch + 7, INT32_MAX, fl, step, false);
            }
            // another step than the kind's: 1 ms off, the opposite sign, one that does not fit 28 bits
            check(epoch, step, epoch + 7, 5, kStPresent, (int64_t)step + 1, false);
            check(epoch, step, epoch + 7, 5, kStPresent, (int64_t)step - 1, false);
            if (step != 0) check(epoch, step, epoch + 7, 5, kStPresent, -(int64_t)step, false);
            check(epoch, step, epoch + 7, 5, kStPresent, 1ll << 27, false);
            check(epoch, step, epoch + 7, 5, kStPresent, 200000000ll, false);
            // no schedule
            check(epoch, step, epoch + 7, 5, 0u, step, false);
        }
    // st_pack_step's own bounds (the wide record's step field)
    EXPECT(st_pack_step((1ll << 27) - 1) && st_step(st_pack_step((1ll << 27) - 1)) == (1ll << 27) - 1);
    EXPECT(st_pack_step(-(1ll << 27)) && st_step(st_pack_step(-(1ll << 27))) == -(1ll << 27));
    EXPECT(!st_pack_step(1ll << 27) && !st_pack_step(-(1ll << 27) - 1));
    // sc_fits at every bound
    EXPECT(sc_fits(0, 0) && sc_fits(top - 1, rhi) && sc_fits(top - 1, rlo));
    EXPECT(!sc_fits(-1, 0) && !sc_fits(top, 0) && !sc_fits(0, rhi + 1) && !sc_fits(0, rlo - 1));
    // every word of a walk across the remain bound and the window's top, as a fire steps them
    {
        const int64_t epoch = 1700000000000ll - kScEpochBack;
        uint64_t w = sc_word(kStPresent | kStForever | kStFired, top - 250, rlo + 2);
        int fires = 0;
        while (true) {
            const int64_t off = sc_off(w) + 100;
            const int32_t rem = sc_remain(w) - 1;
            if (!sc_fits(off, rem)) break;
            w = sc_word((uint32_t)w, off, rem);
            fires++;
            SchedHot h = sc_decode(w, epoch, 100);
            EXPECT(h.next == epoch + off && h.remain == rem && sc_encode(h, epoch, 100, true) == w);
        }
        EXPECT(fires == 2);
    }
    if (fails) {
        printf("%d failures\n", fails);
        return 1;
    }
    printf("sched_word: ok\n");
    return 0;
}
