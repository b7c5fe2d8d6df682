// pool_share.hpp -- the grid of a path_pool launch that shares the device with its caller's other launches (kernel_path_pool.hip,
// launch_path_pool).  No device or HIP dependency: the rule compiles on its own (tests/test_pool_share.py).
//
// drt_renderer_set_frames_in_flight says how many launches the caller KEEPS in flight; how many of them RUN side by side is
// decided by the runtime, which spreads the process's streams over its hardware queues -- GPU_MAX_HW_QUEUES of them, 4 unless the
// environment says otherwise, one of which serves the null stream -- and lets streams that share a queue take turns.  A launch
// that is given 1/hint of the workgroup slots while fewer than `hint` launches run leaves the rest of the chip idle for as long
// as it runs, and a caller that retires its launches in order then waits for the one that is queued behind its queue-mate while
// the streams that have finished stand empty.  So the share is 1 / min(hint, launches that reliably run side by side):
//   * fewer launches in flight than hardware queues: every stream has a queue of its own, the hint is honoured;
//   * as many or more: streams share queues, and what runs side by side reliably is HALF the queues.
// Measured (cornell 1080p / 8 spp, ms per step; one launch at a time on the full grid: 2.70):
//     four in flight, sharing by       1      2      3      4
//     4 queues                       2.75   2.68   3.16   3.87     (four streams on three queues; by 3: three launches open half the time, one a third)
//     8 queues                       2.68   2.53   2.53   2.46     (four streams on four queues)
//     two / three in flight on 4 queues, sharing by the hint: 2.49 / 2.49
// A launch more than fits waits in the dispatcher for the slots its neighbours vacate, which costs nothing; a chip that is a
// quarter empty does.
#pragma once
#include <cstdint>

namespace drt {

// Of `hint` launches in flight, those that reliably run side by side on `hw_queues` hardware queues (<= 0: the runtime's default of 4)
constexpr int pool_share_max(int hint, int hw_queues) {
    const int q = hw_queues > 0 ? hw_queues : 4, h = hint > 1 ? hint : 1;
    return h < q ? h : (q > 1 ? q / 2 : 1);
}

// Workgroups of a launch that wants `want` of the device's `slots` while the caller keeps `hint` launches in flight
constexpr uint64_t pool_shared_grid(uint64_t want, uint64_t slots, int hint, int share_max) {
    const uint64_t h = hint > 1 ? (uint64_t)hint : 1u, m = share_max > 1 ? (uint64_t)share_max : 1u;
    const uint64_t sharers = h < m ? h : m;
    const uint64_t share = (slots + sharers - 1u) / sharers;
    const uint64_t grid = want < share ? want : share;
    return grid > 0u ? grid : 1u;
}

}  // namespace drt
