// Host-only: the switch table of csrc/switches.hpp as this process's environment fills it, one name=value line per switch.
// Built and run by tests/test_switches_cpu.py with plain g++, a fresh process per environment.
#include "switches.hpp"
#include <cstdio>

int main()
{
    const Switches &s = switches();
#define X(type, field, name, kind, value, doc) printf("%s=%lld\n", name, (long long)s.field);
    MAUVE_SWITCHES(X)
#undef X
    return 0;
}
