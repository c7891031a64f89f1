// rec_gate.h -- what the RNN host (rnn_host.h) needs from the residency machinery of
// rec_gate.hip (private to csrc/; the public part is in rnn.h).
#pragma once
#include "rec_common.h"

namespace kctc {

// From a v6 recurrence's launch to the end of the enclosing host call: the
// recurrence this host thread has in flight, and the side streams gated on it.
struct RecScope {
  ~RecScope() { none(); }
  void enqueued(unsigned *flags, int workgroups);  // its flag area (RecParams::flags), dirs * nwg * rg
  void none();  // (also after a generic recurrence: no side launches)
};
// `side` waits until every workgroup of the recurrence in flight is resident;
// whatever is enqueued on it afterwards may run beside that recurrence
void beside_recurrence(hipStream_t side);

// The device's registration word of the exchange's residency gate
// (RecParams::reg) and the registrations expected once every backward
// recurrence enqueued so far is resident
struct RegWord {
  unsigned *word = nullptr;          // [1]: gate timeouts, [2]: pinned XCDs, [4..5]: registrations (64-bit: never wraps),
                                     // [6]: exchange gate blocks gone (rnn_comm_gate)
  unsigned long long expected = 0;   // host: registrations once every enqueued launch is resident
};
RegWord &reg_of_device();

// On s, one wave that returns once each of the `nlines` v6 flag lines from
// `lines` on holds >= epoch, the recurrence reported an error, or after 3 s
// (then err bit 3)
void rec_epoch_gate(hipStream_t s, const unsigned *lines, int nlines, unsigned epoch, unsigned *err);

}  // namespace kctc
