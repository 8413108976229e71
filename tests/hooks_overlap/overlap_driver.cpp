/* overlap_driver.cpp -- TEST INFRASTRUCTURE: the interpreter of overlap_ops.h as a program of its own, for a build with
 * -fsanitize=address,undefined (Makefile: overlap_driver_san). Reads operations (int64 sixes) from the file named first,
 * writes the log (int64 threes) to the file named second. Exit status 0: played; 2: bad arguments or files; 3: a bad operation. */
#include "overlap_ops.h"
#include <stdio.h>

int main(int argc, char **argv) {
	if (argc != 3) return 2;
	FILE *f = fopen(argv[1], "rb");
	if (!f) return 2;
	std::vector<int64_t> ops;
	int64_t buf[6];
	while (fread(buf, sizeof buf, 1, f) == 1) ops.insert(ops.end(), buf, buf + 6);
	fclose(f);
	overlap_ops::Player p;
	if (!p.play(ops.data(), ops.size() / 6)) return 3;
	FILE *g = fopen(argv[2], "wb");
	if (!g) return 2;
	const bool ok = p.log.empty() || fwrite(p.log.data(), sizeof(int64_t), p.log.size(), g) == p.log.size();
	return fclose(g) == 0 && ok ? 0 : 2;
}
