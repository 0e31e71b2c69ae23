// Scan kernel of the lexer (l1_scan.h): the instance for tables of up to 32 passes.
#include "l1_scan.h"

SPA_L1_KERNEL( p32, 32, 256)

namespace spa {
const ScanInstance g_scanInstanceP32 = SPA_L1_SCAN_INSTANCE( 32, 256);
} // namespace
