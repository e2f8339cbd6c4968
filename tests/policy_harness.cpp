// policy_harness.cpp — TEST INFRASTRUCTURE (tests/test_policy_cpu.py): drives the pure frame policies
// of csrc/rtx_policy.h from a script on stdin, one input per line, and prints the policy's whole state
// after each.  Floats go in as C hex floats and come out as their bit patterns, so the traces compare
// exactly with tests/policy_model.py.
//
//   t step BASE MAIN CHAIN | t default | t here | t on 0/1 | t permille P | t rec 0/1
//   w one CRIT RATIO K BEST_SPAN READY ELAPSED | w reset
//   r shape | r upload 0/1 | r set ROUND STATE WAIT QUIET PREV_MAX REC
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <sstream>
#include <string>

#include "rtx_policy.h"

namespace {

unsigned bits(float f) {
    unsigned u;
    std::memcpy(&u, &f, 4);
    return u;
}
float hexf(const std::string& s) { return std::strtof(s.c_str(), nullptr); }

void show(const rtxh::SplitTuner& t) {
    std::printf("t permille=%u on=%d done=%d rec=%d steps=%u dir=%d step=%08x main=%08x chain=%08x best=%08x best_permille=%u\n",
                t.permille, t.on, t.done, t.rec, t.steps, t.dir, bits(t.step_size), bits(t.main_ms), bits(t.chain_ms),
                bits(t.best_span), t.best_permille);
}
void show(const rtxh::InflightWindow& w, int wants, int one) {
    std::printf("w wants=%d one=%d state=%u frames=%u rec=%d interval=%08x\n", wants, one, w.state, w.frames, w.rec,
                bits(w.interval_ms));
}
void show(const rtxh::Refinement& r) {
    std::printf("r round=%u state=%d wait=%u quiet=%u prev_max=%u rec=%d\n", r.round, r.state, r.wait, r.quiet,
                r.prev_max, r.rec);
}

}  // namespace

int main() {
    rtxh::SplitTuner t;
    rtxh::InflightWindow w;
    rtxh::Refinement r;
    char buf[512];
    while (std::fgets(buf, sizeof buf, stdin)) {
        std::istringstream in(buf);
        std::string who, what, a, b, c;
        if (!(in >> who >> what)) continue;
        if (who == "t") {
            unsigned u = 0;
            if (what == "step") {
                in >> u >> a >> b;
                t.step(u, hexf(a), hexf(b));
            } else if (what == "default") t.restart_default();
            else if (what == "here") t.restart_here();
            else if (what == "on") { in >> u; t.on = u != 0; }
            else if (what == "permille") { in >> u; t.permille = u; }
            else if (what == "rec") { in >> u; t.rec = u != 0; }
            else return 2;
            show(t);
        } else if (who == "w") {
            int wants = 0, one = 0;
            if (what == "one") {
                unsigned crit = 0, k = 0, ready = 0;
                in >> crit >> a >> k >> b >> ready >> c;
                wants = w.wants_end(crit, hexf(a));
                one = w.onepiece(crit, hexf(a), k, hexf(b), ready != 0, hexf(c));
            } else if (what == "reset") w.reset();
            else return 2;
            show(w, wants, one);
        } else if (who == "r") {
            unsigned u = 0;
            if (what == "shape") r.reset_shape();
            else if (what == "upload") { in >> u; r.reset_upload(u != 0); }
            else if (what == "set") { in >> r.round >> r.state >> r.wait >> r.quiet >> r.prev_max >> u; r.rec = u != 0; }
            else return 2;
            show(r);
        } else {
            return 2;
        }
    }
    return 0;
}
