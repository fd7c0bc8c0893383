"""GenerationLoader.loadModel (online-local/src/net/myrrix/online/generation/GenerationLoader.java:49-106) restated with
dicts and sets, written from the Java, and the dense form mals_load_generation gives its result (include/myrrix_als.h).

A generation is a dict: X, Y (id -> vector), known (user id -> set of item ids, or None), item_tags (user-side ids),
user_tags (item-side ids).  Python dicts keep insertion order, which is how the live ROW order is carried: the live
generation's dicts are filled in row order, the new model's in the new model's order."""
import numpy as np


def update_tag_ids(current, updated):                      # :108-115
    current |= set(updated)


def update_map(current, updated):                          # :117-126: put
    for key, value in updated.items():
        current[key] = value


def remove_not_updated(container, updated, recently_active):   # :137-152 (a dict's keys, or a set)
    for key in list(container):
        if key not in updated and key not in recently_active:
            if isinstance(container, dict):
                del container[key]
            else:
                container.discard(key)


def load_model(gen, new_x, new_y, updated_known, updated_item_tags, updated_user_tags, recent_users, recent_items,
               remove_not_updated_data=True):
    """loadModel on `gen` in place; recent_users / recent_items (sets) are cleared, as :97-98 do."""
    update_tag_ids(gen["item_tags"], updated_item_tags)                     # :56
    update_tag_ids(gen["user_tags"], updated_user_tags)                     # :57
    update_map(gen["X"], new_x)                                             # :59
    update_map(gen["Y"], new_y)                                             # :60
    if updated_known is not None:                                           # :62-64
        update_map(gen["known"], updated_known)
    updated_x_keys, updated_y_keys = set(new_x), set(new_y)                 # :66-67
    updated_known_users = None if updated_known is None else set(updated_known)
    if remove_not_updated_data:                                             # :72
        remove_not_updated(gen["X"], updated_x_keys, recent_users)          # :74-77
        remove_not_updated(gen["Y"], updated_y_keys, recent_items)          # :78-81
        if updated_known_users is not None and gen["known"] is not None:    # :82-87
            remove_not_updated(gen["known"], updated_known_users, recent_users)
        remove_not_updated(gen["item_tags"], set(updated_item_tags), recent_users)   # :88-91
        remove_not_updated(gen["user_tags"], set(updated_user_tags), recent_items)   # :92-95
    recent_users.clear()                                                    # :97
    recent_items.clear()                                                    # :98
    return gen


def merged_order(live_ids, new_ids, surviving):
    """The dense row order of the merged model: the new rows in the new model's order, then the surviving live rows that
    the new model does not have, in live order."""
    new = set(new_ids)
    return list(new_ids) + [i for i in live_ids if i not in new and i in surviving]


def dense(gen, live_user_ids, live_item_ids, new_user_ids, new_item_ids):
    """The loaded generation as dense arrays in merged row order: dict with user_ids, item_ids, X, Y, known (row_ptr int64,
    item_idx int32, ascending rows), tag_users / tag_items (ascending merged rows), user_map / item_map (live row -> merged
    row, -1 = pruned), n_known_dropped and n_tag_ids_without_row (the one deviation: an id without a merged row is dropped
    from a known-item set or a tag set and counted; the reference keeps the bare id)."""
    uids = merged_order(live_user_ids, new_user_ids, gen["X"])
    iids = merged_order(live_item_ids, new_item_ids, gen["Y"])
    assert set(uids) == set(gen["X"]) and set(iids) == set(gen["Y"])
    urow = {u: r for r, u in enumerate(uids)}
    irow = {i: r for r, i in enumerate(iids)}
    out = {"user_ids": np.array(uids, dtype=np.int64), "item_ids": np.array(iids, dtype=np.int64),
           "X": np.array([gen["X"][u] for u in uids], dtype=np.float32).reshape(len(uids), -1),
           "Y": np.array([gen["Y"][i] for i in iids], dtype=np.float32).reshape(len(iids), -1),
           "user_map": np.array([urow.get(u, -1) for u in live_user_ids], dtype=np.int64),
           "item_map": np.array([irow.get(i, -1) for i in live_item_ids], dtype=np.int64)}
    dropped = 0
    ptr, idx = [0], []
    for u in uids:
        items = (gen["known"] or {}).get(u, ())
        rows = sorted(irow[i] for i in items if i in irow)
        dropped += len(items) - len(rows)
        idx.extend(rows)
        ptr.append(len(idx))
    out["known"] = (np.array(ptr, dtype=np.int64), np.array(idx, dtype=np.int32))
    out["n_known_dropped"] = dropped
    out["tag_users"] = np.array(sorted(urow[t] for t in gen["item_tags"] if t in urow), dtype=np.int64)
    out["tag_items"] = np.array(sorted(irow[t] for t in gen["user_tags"] if t in irow), dtype=np.int64)
    out["n_tag_ids_without_row"] = sum(t not in urow for t in gen["item_tags"]) + sum(t not in irow for t in gen["user_tags"])
    return out


def join(cur_ids, new_ids, recent_rows, keep_not_updated=False):
    """What mals_generation_join_host must return for one side, through load_model on a generation that only has this
    side: (map, counts), or None for a duplicate id (which the dicts cannot hold)."""
    cur_ids, new_ids = [int(i) for i in cur_ids], [int(i) for i in new_ids]
    if len(set(cur_ids)) != len(cur_ids) or len(set(new_ids)) != len(new_ids):
        return None
    gen = {"X": {i: (float(r),) for r, i in enumerate(cur_ids)}, "Y": {}, "known": None, "item_tags": set(), "user_tags": set()}
    recent = {cur_ids[r] for r in recent_rows}
    load_model(gen, {i: (-1.0,) for i in new_ids}, {}, None, set(), set(), recent, set(), not keep_not_updated)
    order = merged_order(cur_ids, new_ids, gen["X"])
    row = {i: r for r, i in enumerate(order)}
    m = np.array([row.get(i, -1) for i in cur_ids], dtype=np.int64)
    new = set(new_ids)
    updated = sum(i in new for i in cur_ids)
    kept = len(order) - len(new_ids)
    return m, {"n_merged": len(order), "n_updated": updated, "n_kept": kept, "n_pruned": len(cur_ids) - updated - kept}
