// Scan kernel of the lexer (l1_scan.h): the instances for tables of 1 to 4 passes.
#include "l1_scan.h"

SPA_L1_KERNEL( p1, 1, 1024)
SPA_L1_KERNEL( p2, 2, 1024)
SPA_L1_KERNEL( p3, 3, 1024)
SPA_L1_KERNEL( p4, 4, 1024)

namespace spa {
const ScanInstance g_scanInstancesP1[ 4] = {
	SPA_L1_SCAN_INSTANCE( 1, 1024), SPA_L1_SCAN_INSTANCE( 2, 1024), SPA_L1_SCAN_INSTANCE( 3, 1024), SPA_L1_SCAN_INSTANCE( 4, 1024)};
} // namespace
