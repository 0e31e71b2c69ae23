// Scan kernel of the lexer (l1_scan.h): the instances for tables of 5 to 8 passes.
#include "l1_scan.h"

SPA_L1_KERNEL( p5, 5, 1024)
SPA_L1_KERNEL( p6, 6, 1024)
SPA_L1_KERNEL( p7, 7, 1024)
SPA_L1_KERNEL( p8, 8, 1024)

namespace spa {
const ScanInstance g_scanInstancesP5[ 4] = {
	SPA_L1_SCAN_INSTANCE( 5, 1024), SPA_L1_SCAN_INSTANCE( 6, 1024), SPA_L1_SCAN_INSTANCE( 7, 1024), SPA_L1_SCAN_INSTANCE( 8, 1024)};
} // namespace
