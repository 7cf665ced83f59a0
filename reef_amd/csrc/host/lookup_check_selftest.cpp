// lookup_check_selftest [lookup|claim|hyrax] -- the lookup leg's checks (lookup_check.hpp) on a tiny honest transcript made on the host
// with plain loops, as a program of its own: no GPU and no libreef_msm.so, so it also runs under host sanitizers.  Prints and exits with
// what reef_replay_lookup_selftest() of libreef_replay.so writes and returns: the JSON line and 0, a rejection and 1, a usage error and 2.
#include "lookup_check.hpp"

int main(int argc, char **argv) {
    (void)&check_selftest;   // proof_check.hpp's own self-test: not this program's
    int rc = 0;
    std::string line;
    try {
        line = lookup_selftest(argc > 1 ? argv[1] : "");
    } catch (const Rejected &e) {
        line = e.what(), rc = 1;
    } catch (const std::exception &e) {
        line = e.what(), rc = 2;
    }
    printf("%s\n", line.c_str());
    return rc;
}
