"""What the tests of the plan as a scan share (tests/test_page_tree_plan.py on the CPU, tests/test_page_tree_plan_gpu.py on the device):
the tables whose rows sit on the seams of zkh_page_tree_plan_device's kernels.  The costs pass takes 256 rows a workgroup, so rows 255
and 256 are the last of one workgroup and the first of the next; the scan of the workgroups' sums takes ceil(workgroups / 256) of them
a lane, so 257 and 513 workgroups are where a lane's chunk grows."""
import numpy as np

SEAM = (10, 500, 8192)                    # h 10, B 16: a part holds its first pair and 6 more nodes
MANY = (10, 500, 8192)                    # every address: 512 pairs of 16 rows, 128 parts of 64 rows, 32 workgroups
WIDE = (12, 200, (1 << 17) + 3)           # every address: 513 workgroups, three sums a lane in the scan; h 15, B 125, 147 parts


def every_address(W):
    return np.arange(W, dtype=np.int64)


def seams():
    """name -> the addresses of a table at SEAM"""
    pairs = lambda qs: [16 * q for q in qs]
    return {
        "rows 255 and 256 in one pair": np.array(pairs(range(256)) + [16 * 255 + 9] + pairs(range(256, 300)), dtype=np.int64),
        "rows 255 and 256 in different pairs": np.array(pairs(range(300)), dtype=np.int64),
        "a part boundary at row 256": every_address(512),                  # parts of 64 rows: one starts at row 256 (the CPU test asserts it)
        "D = 0": np.zeros(0, dtype=np.int64),
        "D = 1": np.array([8191], dtype=np.int64),
        "D = 256": np.array([16 * i + 3 for i in range(256)], dtype=np.int64),
        "D = 257": np.array([16 * i + 3 for i in range(257)], dtype=np.int64),
    }
