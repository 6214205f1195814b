"""The vectors tests/test_exact_sum_model.py checks the accumulator model on and tests/test_exact_sum_host.py replays through the C
header: name -> list of doubles.  q = 2^-192; chunk k of a value has weight 2^(32 k - 192)."""
import math

import numpy as np

ULP63 = 2.0 ** (63 - 53)  # the spacing of doubles just below 2^63


def cases():
    rng = np.random.default_rng(2024)
    out = {}
    out["empty"] = []
    out["one"] = [1.0]
    out["three_chunks"] = [(2.0 ** 53 - 1) * 2.0 ** (-192 + 20)]  # 53 bits from bit 20: chunks 0, 1 and 2
    out["three_chunks_high"] = [-(2.0 ** 53 - 1) * 2.0 ** (-192 + 64 + 31)]
    out["chunk_boundaries"] = [s * 2.0 ** (32 * k - 192) for k in range(8) for s in (1.0, -1.0)] + [2.0 ** (32 * k - 192) for k in range(8)]
    out["below_boundaries"] = [math.nextafter(2.0 ** (32 * k - 192), 0.0) for k in range(1, 8)]
    out["below_q"] = [2.0 ** -193, -(2.0 ** -193), 1.5 * 2.0 ** -192, -1.5 * 2.0 ** -192, 5e-324, 2.0 ** -1000]  # cut toward zero
    out["largest_accepted"] = [2.0 ** 63 - ULP63, -(2.0 ** 63 - ULP63)]
    out["largest_accepted_once"] = [2.0 ** 63 - ULP63]
    out["limit"] = [1.0, 2.0 ** 63]
    out["minus_limit"] = [1.0, -(2.0 ** 63)]
    out["inf"] = [2.0, math.inf]
    out["nan"] = [3.0, math.nan, -math.inf]
    out["alternating_largest_chunk"] = [(1.0 if i % 2 == 0 else -1.0) * (2.0 ** 32 - 1) * 2.0 ** (32 * 3 - 192) for i in range(1 << 16)]
    out["same_sign_largest_chunk"] = [(2.0 ** 32 - 1) * 2.0 ** (32 * 2 - 192)] * (1 << 16)
    out["cancels_to_zero"] = [0.1, 0.2, -0.1, 1e10, -0.2, -1e10]
    out["negative_total"] = [0.1, -0.3, 2.0 ** -60]
    out["tie_to_even_down"] = [1.0, 2.0 ** -53]            # 1 + half an ulp: the even neighbour is 1
    out["tie_to_even_up"] = [1.0 + 2.0 ** -52, 2.0 ** -53]  # (1 + ulp) + half an ulp: the even neighbour is 1 + 2 ulp
    out["above_tie"] = [1.0, 2.0 ** -53, 2.0 ** -150]       # a sticky bit far below decides
    out["carry_into_new_bit"] = [2.0 - 2.0 ** -52, 2.0 ** -53]  # rounds up to 2
    out["wide_range"] = [float(v) for v in rng.standard_normal(300) * 10.0 ** rng.uniform(-30, 15, 300)]
    out["unit_scale"] = [float(v) for v in rng.standard_normal(1000)]
    return out
