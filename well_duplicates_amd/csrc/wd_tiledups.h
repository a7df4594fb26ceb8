// wd_tiledups.h - what welldup_tiledups.hip shares with welldup_core.hip.  Kept out of wd_ctx.h, which
// every unit includes: the other units' sources, and with them their unit ids, stay as they are.
#ifndef WD_TILEDUPS_H
#define WD_TILEDUPS_H

namespace wd {
const char *unit_id_tiledups();      // hash of the tiledups unit's sources (wd_build_id)
}

#endif
