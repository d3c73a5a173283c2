"""The smallest shapes that reach the code paths 1080p and 4K frames take in csrc/frame_result.hip and csrc/merge.hip.
The -m gpu tests (test_gpu_o_frame_result.py, test_gpu_c_bank.py) run them on the device; test_frame_result_cpu.py
pins each one to its path from the launchers' own arithmetic, so that a change of a range, a table size or a grid cap
cannot leave the device tests passing on shapes that no longer reach anything.

`rle_plan` gives a workgroup a range of max(512, ceil(total / (2^22 / channels))) positions, rounded up to 64; `groups`
is the number of ranges, and each of the 256 threads of `rle_scan_kernel` scans chunk = ceil(groups / 256) entries."""

# (h, w, channels of the hand-built planes' tables, groups, chunk): 512-position ranges
RLE_ONE_ENTRY = (270, 480, 254, 1)      # the largest plane the suite had: every thread at most one table entry
RLE_TWO_ENTRIES = (300, 480, 282, 2)    # threads 0..140 hold two entries each, 115 threads are idle
RLE_PARTIAL_CHUNK = (526, 750, 771, 4)  # threads 0..191 hold four, thread 192 holds three, 63 threads are idle
# 4096 channels leave 2^22 / 4096 = 1024 ranges at most: ceil(544000 / 1024) = 532 -> 576 positions per range
RLE_GROWN_RANGE = (544, 1000, 945, 4)
RLE_GROWN_CHANNELS = 4096

# `frame_result`: output sizes whose 4-pixel groups outnumber the threads of the capped grid
FRAME_PROB = (3, 57, 64)
FRAME_PACKED = (2052, 2048)     # 512 groups per row, 1 050 624 in all, the packed stores
FRAME_ELEMENTWISE = (2052, 2050)  # 513 groups per row, 1 052 676 in all, a 2-pixel last group, element-wise stores

# `lut_remap`, `merge_paint`, `label_histogram`: one pixel per thread and step
MERGE_LARGE = (1025, 2049)      # 2 100 225 pixels
