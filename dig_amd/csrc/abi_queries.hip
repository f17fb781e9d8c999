// The host-only queries both builds answer alike (abi_queries.inc); no device code.
#include <algorithm>
#include <vector>
#include "abi_rules.h"
#include "abi_queries.inc"
