/*
 * Stand-alone driver for the host arithmetic of the packed Q1 companion
 * (greengage_amd/csrc/q1_pack.h), built and run by test_q1_pack_cpu.py.
 * One query per input line, one answer per output line:
 *   E n qmin qmax pmin pmax dmin dmax tmin tmax sdmin sdmax -> 0 | 1
 *   B pmax tmax          -> row bound
 *   G n want row_bound   -> grid rows_per_block grid_ok
 *   C cutoff sd_base     -> -1 (no row passes) | c
 */
#include <cinttypes>
#include <cstdio>
#include <cstring>

#include "../greengage_amd/csrc/q1_pack.h"

int main()
{
	char line[512];

	while (fgets(line, sizeof line, stdin))
	{
		long long a[11];
		unsigned long long u;

		if (line[0] == 'E' &&
		    sscanf(line + 1, "%lld %lld %lld %lld %lld %lld %lld %lld "
			   "%lld %lld %lld", &a[0], &a[1], &a[2], &a[3], &a[4],
			   &a[5], &a[6], &a[7], &a[8], &a[9], &a[10]) == 11)
		{
			gg::Q1PackRanges r = {a[1], a[2], a[3], a[4], a[5],
					      a[6], a[7], a[8], a[9], a[10]};

			printf("%d\n", (int) gg::q1_pack_eligible(a[0], r));
		}
		else if (line[0] == 'B' &&
			 sscanf(line + 1, "%lld %lld", &a[0], &a[1]) == 2)
			printf("%" PRIu64 "\n",
			       gg::q1_pack_row_bound(a[0], a[1]));
		else if (line[0] == 'G' &&
			 sscanf(line + 1, "%lld %lld %llu", &a[0], &a[1],
				&u) == 3)
		{
			int64_t g = gg::q1_pack_grid(a[0], a[1], u);

			printf("%" PRId64 " %" PRId64 " %d\n", g,
			       gg::q1_pack_rows_per_block(a[0], g),
			       (int) gg::q1_pack_grid_ok(a[0], g, u));
		}
		else if (line[0] == 'C' &&
			 sscanf(line + 1, "%lld %lld", &a[0], &a[1]) == 2)
		{
			uint32_t c = 0;

			if (gg::q1_pack_cutoff((int32_t) a[0], (int32_t) a[1],
					       &c))
				printf("%u\n", c);
			else
				printf("-1\n");
		}
		else
		{
			fprintf(stderr, "bad query: %s", line);
			return 2;
		}
	}
	return 0;
}
