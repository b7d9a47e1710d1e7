// le_ctrack.hip -- the LE Coded connection tracking as a translation unit of its own (le_ctrack.h says why)
#include "le_ctrack.h"
