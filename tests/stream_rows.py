"""Cases for the lane-per-row forms of the quotient and row-sum kernels (csrc/stark.hip quotient_stream_kernel, rowdot_stream_kernel): a
wavefront stages 64 rows through LDS in slices of 32 columns and every lane sums its own row.  Shared by test_stream_rows_cpu.py and
test_gpu_stream_rows.py (no GPU and no library call here).

Dispatch (mirrors of launch_rowdot and launch_quotient; the 16-lane forms serve every other shape):

  row sums   rowdot_form(width, rows) in 1..4 (so what zkhip_reduced_opening reports does not change) and width % 32 == 0 and
             rows % 64 == 0 and rows >= 2048
  quotient   width % 32 == 0 and 2N >= 2048

zkhip_reduced_opening takes log_rows, so through it the row count is a power of two: "one workgroup (256 rows) below the threshold" is
not reachable, the case below the threshold is 2^10 rows, and no launch ends in a partial workgroup (the kernel's wavefronts check
their first row all the same).
"""
import reduced_edges as RE

SLICE_COLS = 32
STREAM_MIN_ROWS = 2048
ROWS_PER_WORKGROUP = 256


def rowdot_stream_form(width, rows):
    return RE.rowdot_form(width, rows) != 0 and width % SLICE_COLS == 0 and rows % 64 == 0 and rows >= STREAM_MIN_ROWS


def quotient_stream_form(log_n, width):
    return width % SLICE_COLS == 0 and (2 << log_n) >= STREAM_MIN_ROWS


# reduced_edges.CASES layout: (id, log_rows, width, padded, p_width, q_width, accumulate, form of the trace block, form of the permutation block or -1),
# then whether the trace block / the permutation block takes the lane-per-row form (literals, held against the mirror above by test_stream_rows_cpu.py)
#   thr: 2048 rows, the threshold; below: 1024 rows, the 16-lane form; two: 8192 rows, 32 workgroups
#   widths 32 (one slice, eight lanes per row in the 16-lane form), 96 (three slices), 256 (eight slices: the headline width)
#   fall: widths inside forms 1..4 that are no multiple of 32 keep the 16-lane form at any height
#   padded 1: the block starts 4 columns into rows of pitch width + 8, so rows are 16-byte but not 128-byte aligned
ROWDOT_CASES = (
    (("thr-32x2^11", 11, 32, 0, 0, 0, 0, 1, -1), True, False),
    (("below-32x2^10", 10, 32, 1, 32, 8, 0, 1, 1), False, False),
    (("thr-96x2^11", 11, 96, 1, 32, 8, 1, 2, 1), True, True),
    (("below-96x2^10", 10, 96, 0, 0, 16, 0, 2, -1), False, False),
    (("thr-256x2^11", 11, 256, 1, 8, 16, 0, 4, 1), True, False),
    (("below-256x2^10", 10, 256, 0, 256, 0, 1, 4, 4), False, False),
    (("two-256x2^13", 13, 256, 0, 96, 8, 1, 4, 2), True, True),
    (("fall-68x2^11", 11, 68, 0, 100, 8, 0, 2, 2), False, False),
    (("fall-240x2^12", 12, 240, 1, 260, 0, 0, 4, 0), False, False),
)

# (log_n, width): the quotient of the synthetic AIR over 2N rows; all take the lane-per-row form.  Every row of both chunks is compared, which
# includes the last wavefront of each chunk, whose 65th row wraps to e = parity.
QUOTIENT_CASES = ((10, 32), (11, 96), (12, 256))
QUOTIENT_FALLBACK = ((10, 48), (9, 32))            # no whole slices; under the threshold

# whole proofs at 2^10 x 32 (quotient and trace row sums in the lane-per-row forms): LogUp pairs 0 / 2 (the addend table added per lane), blowup 2 (the
# quotient value also goes straight into the quotient LDE: lde_out) and blowup 4 (it does not): (log_blowup, queries, pow_bits, pairs)
PROOF_CASES = ((1, 8, 4, 0), (1, 8, 4, 2), (2, 8, 4, 0), (2, 8, 4, 2))
