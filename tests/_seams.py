"""Where the scan kernels hand work out, shared by the seam test of test_gpu_scan.py and the far capture of _far.py
(test infrastructure): scan_known_lap_kernel gives a lane a run of two words (128 offsets), a segment 4096 offsets, a wave 128
words and a tile 512 words; scan_slide_kernel a word, a wave 63 words and a tile 756 words."""

# a sync word begins this many bits from a seam: right before, on and behind it, and with windows that straddle it
DELTAS = (-65, -64, -63, -33, -32, -31, -1, 0, 1, 31, 32, 33, 63, 64)
# the seams, in words from the start of a stream
BOUNDS = (1, 2, 63, 64, 126, 128, 189, 256, 512, 756, 1024, 1512)
# two tiles of each kernel and a ragged rest
N_WORDS = 2 * 512 + 2 * 756 + 37
