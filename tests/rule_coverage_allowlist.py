"""The branches of the oracle's rule functions that no reference-recorded fixture takes (tests/test_rule_coverage_cpu.py asserts
that this list EQUALS what `gcc -O0 --coverage` + gcov measure).  Entries: (function, stripped source line, occurrence of that line's
text within the function, branch index on the line as gcov numbers it, reason why no legal play reaches it).  A branch belongs here only
when no game played through the reference's validate_action can take it; everything else needs a fixture under tests/golden/."""

NEVER_TAKEN = [
    ("valid_dev_cards", "if (c == C_YOP) { if (banksum > 0) cards5[c] = 1.0f; }", 0, 3,
     "Year of Plenty in hand while the WHOLE bank is empty: all 95 resource cards would have to sit in the four hands at once, and every "
     "7 halves a hand above 7; no game from reset gets there and the reference cannot import a state (a bank short of SOME resource is "
     "traj_rule_yop_bank_short)"),
    ("orc_masks", "if (r & 1) {", 0, 1,
     "before the roll nothing was bought this turn (bought_this_turn is cleared by EndTurn and buying needs the roll), so every hidden "
     "card is playable; only Year of Plenty with the whole bank empty (above) could leave none"),
    ("orc_masks", "if (ag && ar) { m[M0 + T_EXCHANGE] = 1.0f; for (int i = 0; i < 5; i++) { m[M9 + i] = give[i]; m[M10 + i] = recv[i]; } }", 0, 3,
     "something to give but NO bank resource to receive: the whole bank empty again (see valid_dev_cards)"),
    ("update_players_go", "if (left) { if (--e->player_order_id < 0) e->player_order_id = 3; }", 0, 2,
     "the turn moves left only in the second placement round, from seat 3 down to seat 0 (game.py:253-262, 575-590); the road of seat 0 "
     "ends the phase without moving, so the index never wraps below 0"),
    ("orc_step", "switch (type) {", 0, 13,
     "the default label: an action type outside 0..12 never reaches the step, validate_action rejects it first (the rejection itself is "
     "pinned by the out_of_range probes of validate_cases.npz through orc_action_is_legal)"),
    ("orc_step", "for (int i = 0; i < 5; i++) { if (k < v->res[order[i]]) { r = order[i]; break; } k -= v->res[order[i]]; }", 0, 3,
     "the loop running out: k is drawn below the victim's total hand, so one of the five resources always holds card k"),
    ("orc_step", "for (int i = 0; i < pl->n_hidden; i++) if (pl->hidden[i] == card) { at = i; break; }", 0, 3,
     "the loop running out: validate_action accepts PlayDevelopmentCard only for a card in the hidden hand (game.py:403)"),
    ("orc_step", "if (at >= 0) {", 0, 1,
     "the played card not found in the hidden hand: same reason as the search loop above"),
    ("orc_step", "} else if (card == C_YOP) {", 0, 1,
     "the last of five card kinds: after victory point, knight, road building and monopoly only Year of Plenty is left"),
]
