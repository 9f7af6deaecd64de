// Host build of csrc/t4d_repr.h for the CPU tests: reads raw float64 values from stdin, writes one repr per line to stdout.
#include <stdio.h>

#include "../../topo4d_amd/csrc/t4d_repr.h"

int main()
{
    double x;
    char buf[T4D_REPR_MAX_CHARS + 1];
    while (fread(&x, sizeof x, 1, stdin) == 1) {
        const int n = t4d_repr::format(x, buf);
        buf[n] = '\n';
        fwrite(buf, 1, (size_t)n + 1, stdout);
    }
    return 0;
}
