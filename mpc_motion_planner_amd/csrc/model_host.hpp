// model_host.hpp — what the C-ABI unit (mpcmp.hip) uses of the host-only file model_host.cpp besides the entry points of include/mpcmp.h: the
// checks of a configuration, a bound row and a payload, and the error text of calls that have no context.  Plain C++ (no HIP header).
#pragma once
#include <string>
#include "../../include/mpcmp.h"

namespace mpcmp {

// the message of the last failed call of this thread that had no context to keep it in (mpcmp_last_error(NULL))
extern thread_local std::string g_err;

// MPCMP_OK, or MPCMP_EINVAL with the reason in err
int validate(const mpcmp_config *c, std::string &err);
int validate_boxes(const mpcmp_bounds *t, std::string &err);
int validate_general_rows(const mpcmp_bounds *t, int num_seg, std::string &err);
int check_payload(const mpcmp_payload *p, std::string &err);

}  // namespace mpcmp
