// kernels_search_temporal.hip -- k_search_rows / k_search_step with a table of temporal candidates (havoc_mi355x_search_temporal): kernels_search.hip compiled once
// more for those instantiations alone (launch_search_walk_temporal), so that the kernels without a table are compiled without them and stay the code they were.
#define HAVOC_SEARCH_TEMPORAL_UNIT 1
#include "kernels_search.hip"
