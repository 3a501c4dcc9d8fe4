/*
 * Stand-alone driver for the host arithmetic of the 8 B tier of the packed
 * Q1 companion (greengage_amd/csrc/q1_pack.h), built and run by
 * test_q1_pack8_cpu.py.  One query per input line, one answer per line;
 * R stands for the ranges "qmin qmax pmin pmax dmin dmax tmin tmax sdmin
 * sdmax":
 *   W R            -> width sum in bits
 *   E n R          -> 0 | 1 (8 B tier eligible)
 *   L R            -> sd_mask code_shift d_shift d_mask t_shift t_mask
 *                     q_shift q_mask p_shift p_mask bits
 *   P R sd code d t q p -> the packed word, then the six fields unpacked
 *                     from it: word sd code d t q p
 *   C cutoff sd_base sd_mask -> -1 (no row passes) | c
 *   G n want row_bound   -> grid (q1_pack_grid, shared with the 12 B tier)
 *   F n grid qmax dmax   -> rows_per_replica on d_shift (Q1Pack8Fold)
 */
#include <cinttypes>
#include <cstdio>
#include <cstring>

#include "../greengage_amd/csrc/q1_pack.h"

static gg::Q1PackRanges ranges(const long long *a)
{
	gg::Q1PackRanges r = {a[0], a[1], a[2], a[3], a[4],
			      a[5], a[6], a[7], a[8], a[9]};

	return r;
}

#define R10 "%lld %lld %lld %lld %lld %lld %lld %lld %lld %lld"
#define A10(a, o) &a[o], &a[o + 1], &a[o + 2], &a[o + 3], &a[o + 4], \
	&a[o + 5], &a[o + 6], &a[o + 7], &a[o + 8], &a[o + 9]

int main()
{
	char line[1024];

	while (fgets(line, sizeof line, stdin))
	{
		long long a[17];
		unsigned long long u;

		if (line[0] == 'W' && sscanf(line + 1, R10, A10(a, 0)) == 10)
			printf("%d\n", gg::q1_pack8_width(ranges(a)));
		else if (line[0] == 'E' &&
			 sscanf(line + 1, "%lld " R10, &a[0], A10(a, 1)) == 11)
			printf("%d\n", (int) gg::q1_pack8_eligible(
				       a[0], ranges(a + 1)));
		else if (line[0] == 'L' &&
			 sscanf(line + 1, R10, A10(a, 0)) == 10)
		{
			gg::Q1Pack8Layout l = gg::q1_pack8_layout(ranges(a));

			printf("%u %u %u %u %u %u %u %u %u %u %u\n", l.sd_mask,
			       l.code_shift, l.d_shift, l.d_mask, l.t_shift,
			       l.t_mask, l.q_shift, l.q_mask, l.p_shift,
			       l.p_mask, l.bits);
		}
		else if (line[0] == 'P' &&
			 sscanf(line + 1, R10 " %lld %lld %lld %lld %lld %lld",
				A10(a, 0), &a[10], &a[11], &a[12], &a[13],
				&a[14], &a[15]) == 16)
		{
			gg::Q1Pack8Layout l = gg::q1_pack8_layout(ranges(a));
			unsigned long long w = gg::q1_pack8_word(
				l, (uint32_t) a[10], (uint32_t) a[11],
				(uint32_t) a[12], (uint32_t) a[13],
				(uint32_t) a[14], (uint32_t) a[15]);

			printf("%llu %u %u %u %u %u %u\n", w,
			       gg::q1_pack8_sd(l, w), gg::q1_pack8_code(l, w),
			       gg::q1_pack8_disc(l, w), gg::q1_pack8_tax(l, w),
			       gg::q1_pack8_qty(l, w),
			       gg::q1_pack8_price(l, w));
		}
		else if (line[0] == 'C' &&
			 sscanf(line + 1, "%lld %lld %lld", &a[0], &a[1],
				&a[2]) == 3)
		{
			uint32_t c = 0;

			if (gg::q1_pack8_cutoff((int32_t) a[0], (int32_t) a[1],
						(uint32_t) a[2], &c))
				printf("%u\n", c);
			else
				printf("-1\n");
		}
		else if (line[0] == 'G' &&
			 sscanf(line + 1, "%lld %lld %llu", &a[0], &a[1],
				&u) == 3)
			printf("%" PRId64 "\n", gg::q1_pack_grid(a[0], a[1], u));
		else if (line[0] == 'F' &&
			 sscanf(line + 1, "%lld %lld %lld %lld", &a[0], &a[1],
				&a[2], &a[3]) == 4)
		{
			gg::Q1Pack8Fold f = gg::q1_pack8_fold(a[0], a[1], a[2],
							      a[3]);

			printf("%" PRId64 " %u %u\n",
			       gg::q1_pack8_rows_per_replica(a[0], a[1]), f.on,
			       f.d_shift);
		}
		else
		{
			fprintf(stderr, "bad query: %s", line);
			return 2;
		}
	}
	return 0;
}
