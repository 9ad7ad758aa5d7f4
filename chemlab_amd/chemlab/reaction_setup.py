"""Reaction dict (reaction_parser) -> espressopp-shaped objects: one ChemicalReaction, one
FixedPairList + bond interaction per group, one Reaction per equation, type change post-process.
Behaviour of /root/reference/src/chemlab/reaction_setup.py:71-165,408-541 (normal reactions)."""


class SetupReactions(object):
    def __init__(self, espressopp, system, vl, topol, topol_manager, config, args=None):
        self.espp, self.system, self.vl, self.topol, self.tm, self.cfg, self.args = espressopp, system, vl, topol, topol_manager, config, args
        self.name2type = topol.used_atomsym_atomtype
        self.dynamic_types = set()
        self.fpls = []
        self.extensions_to_integrator = []
        self.fix_distances = []            # FixDistances objects of ReleaseMolecule extensions
        self.use_thermal_group = False     # set by an extension that adds particles the thermostat must leave alone

    def _setup_reaction_normal(self, cr, fpl):
        e, rl = self.espp, cr["reactant_list"]
        n2t = self.name2type
        r_class = e.integrator.RestrictReaction if cr.get("connectivity_map") else e.integrator.Reaction      # reaction_setup.py:75-78
        r = r_class(
            type_1=n2t[rl["type_1"]["name"]], type_2=n2t[rl["type_2"]["name"]],
            delta_1=int(rl["type_1"]["delta"]), delta_2=int(rl["type_2"]["delta"]),
            min_state_1=int(rl["type_1"]["min"]), max_state_1=int(rl["type_1"]["max"]),
            min_state_2=int(rl["type_2"]["min"]), max_state_2=int(rl["type_2"]["max"]),
            rate=float(cr["rate"]), fpl=fpl, cutoff=float(cr["cutoff"]))
        self.dynamic_types.update((r.type_1, r.type_2))
        r.intramolecular = bool(cr["intramolecular"])
        r.intraresidual = bool(cr["intraresidual"])
        r.is_virtual = bool(cr["virtual"])
        if "min_cutoff" in cr:
            r.get_reaction_cutoff().min_cutoff = float(cr["min_cutoff"])
        r.active = cr.get("active", True)
        if cr.get("connectivity_map"):                       # id pairs `b1 b2`, one per line (reaction_setup.py:115-128)
            conn = set()
            with open(cr["connectivity_map"]) as f:
                for line in f:
                    if line.strip():
                        b1, b2 = map(int, line.split())
                        conn.add(tuple(sorted((b1, b2))))
            for b1, b2 in sorted(conn):
                r.define_connection(b1, b2)
        for which in ("type_1", "type_2"):
            old, new = rl[which]["name"], rl[which]["new_type"]
            if old != new:   # type change with the new type's mass and charge from [ atomtypes ]
                pp = e.integrator.PostProcessChangeProperty()
                prop = self.topol.gt.atomtypes[new]
                pp.add_change_property(n2t[old], e.integrator.TopologyParticleProperties(type=n2t[new], mass=prop["mass"], q=prop["charge"]))
                r.add_postprocess(pp, which)
                self.dynamic_types.update((n2t[old], n2t[new]))
        return r

    def _setup_reaction_dissociation(self, cr, fpl):
        """`A(a,b):B(c,d) -> A'(x) + B'(y)` with `alpha` (reaction_setup.py:257-356): on the break both particles get
        lambda_adr = 0 and keep their type; BasicDynamicResolution({t1_old: alpha, t2_old: alpha}) ramps them, and its
        post-process changes type, mass and charge when lambda is back at 1.  The broken bonds are those of the group's list."""
        e, rl, n2t = self.espp, cr["reactant_list"], self.name2type
        if cr.get("connectivity_map"):
            raise RuntimeError("connectivity_map not supported by dissociation reaction")
        t1_old, t1_new = n2t[rl["type_1"]["name"]], n2t[rl["type_1"]["new_type"]]
        t2_old, t2_new = n2t[rl["type_2"]["name"]], n2t[rl["type_2"]["new_type"]]
        r = e.integrator.DissociationReaction(
            type_1=t1_old, type_2=t2_old, delta_1=int(rl["type_1"]["delta"]), delta_2=int(rl["type_2"]["delta"]),
            min_state_1=int(rl["type_1"]["min"]), max_state_1=int(rl["type_1"]["max"]),
            min_state_2=int(rl["type_2"]["min"]), max_state_2=int(rl["type_2"]["max"]),
            rate=float(cr["rate"]), fpl=fpl, cutoff=float(cr["cutoff"]))
        if "diss_rate" in cr:
            r.diss_rate = cr["diss_rate"]
        r.active = cr.get("active", True)
        if "min_cutoff" in cr:
            r.get_reaction_cutoff().min_cutoff = float(cr["min_cutoff"])
        r.is_virtual = bool(cr["virtual"])
        self.dynamic_types.update((t1_old, t2_old, t1_new, t2_new))
        alpha = float(cr["alpha"])
        dyn_res = e.integrator.BasicDynamicResolution(self.system, {t1_old: alpha, t2_old: alpha})
        for which, old, new, new_name in (("type_1", t1_old, t1_new, rl["type_1"]["new_type"]), ("type_2", t2_old, t2_new, rl["type_2"]["new_type"])):
            if old != new:
                prop = self.topol.gt.atomtypes[new_name]
                tpp = e.integrator.TopologyParticleProperties(type=new, mass=prop["mass"], lambda_adr=1.0, q=prop["charge"])
                dyn_res.add_postprocess(e.integrator.PostProcessChangeProperty(old, tpp))
            r_pp = e.integrator.PostProcessChangeProperty()
            r_pp.add_change_property(old, e.integrator.TopologyParticleProperties(lambda_adr=0.0))
            r.add_postprocess(r_pp, which)
        self.extensions_to_integrator.append(dyn_res)
        return r

    def _setup_reaction_exchange(self, cr, fpl):
        """`A:B + C -> A:C + B` (reaction_setup.py:167-251): a VIRTUAL A + C reaction -- no bond is made or removed, the event
        only changes properties -- that requires A to carry a bonded B in B's state window; A changes type like a normal
        reactant, the B neighbours of A in the window take B's new type and have their state incremented."""
        e, rl, n2t = self.espp, cr["reactant_list"], self.name2type
        if cr.get("connectivity_map"):
            raise RuntimeError("connectivity_map not supported by exchange reaction")
        rt1, rt2, rt3 = rl["type_1"], rl["type_2"], rl["type_3"]
        r = e.integrator.Reaction(
            type_1=n2t[rt1["name"]], type_2=n2t[rt3["name"]], delta_1=int(rt1["delta"]), delta_2=int(rt3["delta"]),
            min_state_1=int(rt1["min"]), max_state_1=int(rt1["max"]), min_state_2=int(rt3["min"]), max_state_2=int(rt3["max"]),
            rate=float(cr["rate"]), fpl=fpl, cutoff=float(cr["cutoff"]))
        r.is_virtual = True
        r.add_constraint(e.integrator.ReactionConstraintNeighbourState(n2t[rt2["name"]], int(rt2["min"]), int(rt2["max"])), "type_1")
        r.intraresidual = bool(cr["intraresidual"])
        r.intramolecular = bool(cr["intramolecular"])
        if "min_cutoff" in cr:
            r.get_reaction_cutoff().min_cutoff = float(cr["min_cutoff"])
        r.active = cr.get("active", True)
        t1_old, t1_new = n2t[rt1["name"]], n2t[rt1["new_type"]]
        t2_old, t2_new = n2t[rt2["name"]], n2t[rt2["new_type"]]
        self.dynamic_types.update((t1_old, t1_new, t2_old, t2_new, n2t[rt3["name"]]))
        if t1_old != t1_new:
            pp = e.integrator.PostProcessChangePropertyByTopologyManager(self.tm)
            prop = self.topol.gt.atomtypes[rt1["new_type"]]
            pp.add_change_property(t1_old, e.integrator.TopologyParticleProperties(type=t1_new, mass=prop["mass"], q=prop["charge"]))
            r.add_postprocess(pp, "type_1")
        prop = self.topol.gt.atomtypes[rt2["new_type"]]
        tpp = e.integrator.TopologyParticleProperties(type=t2_new, mass=prop["mass"], q=prop["charge"], incr_state=int(rt2["delta"]))
        tpp.set_min_max_state(int(rt2["min"]), int(rt2["max"]))
        nb = e.integrator.PostProcessChangeNeighboursProperty(self.tm)
        nb.add_change_property(t2_old, tpp, 1)
        r.add_postprocess(nb, "type_1")
        return r

    def _setup_extension(self, name):
        """[ext_<name>] -> (post-process object, invoke_on).  In scope: ChangeNeighboursProperty
        (reaction_post_process.py:76-115: `type_transfers=OLD:level->NEW[(state=1,...)],...`)."""
        import re
        cfg = self.cfg["extensions"].get(name)
        if cfg is None:
            raise RuntimeError("extension %s is not defined ([ext_%s] missing)" % (name, name))
        if cfg.get("ext_type") == "ATRPActivator":
            return self._setup_atrp_activator(cfg), None
        if cfg.get("ext_type") == "ReleaseMolecule":
            return self._setup_release_molecule(cfg)
        if cfg.get("ext_type") in ("JoinMolecule", "RemoveNeighboursBonds"):
            # The engine is asked first, before anything of the section is parsed: the CPU checker has no reverse reactions
            # and answers with NotImplementedError naming the extension, whatever keys the section holds.
            if not self.system.engine.supports("reaction_join" if cfg["ext_type"] == "JoinMolecule" else "reaction_remove_bond"):
                raise NotImplementedError("reaction extension %s (%s): the CPU checker has no reverse reactions" % (name, cfg["ext_type"]))
            return self._setup_join_molecule(cfg) if cfg["ext_type"] == "JoinMolecule" else self._setup_remove_neighbour_bonds(cfg)
        if cfg.get("ext_type") in ("FreezeRegion", "ChangeParticleType"):
            # asked first, as for JoinMolecule: the CPU checker has no region rules, whatever keys the section holds
            if not self.system.engine.supports("region"):
                raise NotImplementedError("reaction extension %s (%s): the CPU checker has no region rules" % (name, cfg["ext_type"]))
            return self._setup_freeze_region(cfg) if cfg["ext_type"] == "FreezeRegion" else (self._setup_change_particle_type(cfg), None)
        if cfg.get("ext_type") != "ChangeNeighboursProperty":
            raise NotImplementedError("reaction extension %s (%s) is outside the hot-path scope (SURVEY f-4)" % (name, cfg.get("ext_type")))
        e, n2t = self.espp, self.name2type
        pp = e.integrator.PostProcessChangeNeighboursProperty(self.tm)
        re_opt = re.compile(r"(?P<type_name>\w+)\(?(?P<options>[a-zA-Z0-9_=,]*)\)?")
        for tr in cfg["type_transfers"].split(","):
            old, new = tr.split("->")
            old_type, nb_level = old.split(":")
            new_type, options = re_opt.match(new).groups()
            prop = self.topol.gt.atomtypes[new_type]
            if "state" not in prop:
                raise RuntimeError("Please define initial atom state in [ atomstate ] section of your topology for atom type %s" % new_type)
            kw = dict(type=n2t[new_type], mass=prop["mass"], q=prop["charge"], state=prop["state"])
            for kv in filter(None, options.split(",")):
                k, v = kv.split("=")
                kw[k] = int(v) if k in ("state", "type") else float(v)
            pp.add_change_property(n2t[old_type], e.integrator.TopologyParticleProperties(**kw), int(nb_level))
            self.dynamic_types.update((n2t[old_type], n2t[new_type]))
        return pp, cfg.get("invoke_on", "both")

    def _setup_release_molecule(self, cfg):
        """[ext_*] ext_type=ReleaseMolecule (reaction_post_process.py:203-320): every particle of `host_type` gets `replicate`
        dummy particles of a new type at `eq_length`, held there by FixDistances; a bond of the host (`release_on=bond`,
        `release_count` per event) or a type change of host or dummy (`release_on=type`) sets a dummy free as `target_type` at
        lambda 0, BasicDynamicResolution({target: alpha}) fades it in and, where `final_type` differs, changes it once more at
        lambda 1.  Returns (PostProcessReleaseParticles | None, invoke_on)."""
        e, topol = self.espp, self.topol
        host_type, target_type = cfg["host_type"], cfg["target_type"]
        eq_length, alpha, init_res = float(cfg["eq_length"]), float(cfg["alpha"]), float(cfg["init_res"])
        final_type = cfg.get("final_type", target_type)
        if cfg.get("cache_file"):
            raise NotImplementedError("ReleaseMolecule cache_file is a Python 2 pickle of the reference's own objects: not read or written here")
        replicate = int(cfg.get("replicate", 1))
        release_on = cfg.get("release_on", "type")
        if release_on not in ("bond", "type"):
            raise RuntimeError("Wrong keyword release_on %s, only: bond or type" % release_on)
        release_count = int(cfg.get("release_count", 1))
        invoke_on = cfg.get("invoke_on", "both")        # (the reference reads invoke_on: a `release_host=` key has no effect there, nor here)
        if invoke_on not in ("type_1", "type_2", "both"):
            raise RuntimeError("Wrong keyword invoke_on %s, only type_1, type_2, both" % invoke_on)
        dummy_type_id = max(topol.atomsym_atomtype.values()) + 1
        topol.add_new_atomtype(dummy_type_id, "DUMMY_%d" % dummy_type_id, False)
        host_pids = sorted(pid for pid, v in topol.atoms.items() if v["type"] == host_type)
        target_type_id = topol.atomsym_atomtype[target_type]
        target_properties = topol.gt.atomtypes[target_type]
        eng = self.system.engine
        ids, pos = eng.get_state("ID"), eng.get_state("POS")
        row = {int(pid): k for k, pid in enumerate(ids.tolist())}
        particle_list, fix_list = [], []
        dummy_idx = max(topol.atoms) + 1
        for host_pid in host_pids:
            hp = pos[row[host_pid]]
            for _ in range(replicate):
                fix_list.append((host_pid, dummy_idx, eq_length))
                particle_list.append([dummy_idx, dummy_type_id, e.Real3D(hp[0] + eq_length, hp[1], hp[2]), target_properties["mass"], dummy_idx,
                                      init_res, target_properties.get("state", 0)])
                dummy_idx += 1
        self.system.storage.addParticles(particle_list, "id", "type", "pos", "mass", "res_id", "lambda_adr", "state")
        self.system.storage.decompose()
        release_pp = None
        if release_on == "type":
            fd = e.integrator.FixDistances(self.system, fix_list, topol.atomsym_atomtype[host_type], dummy_type_id)
        else:
            fd = e.integrator.FixDistances(self.system, fix_list)
            release_pp = e.integrator.PostProcessReleaseParticles(fd, release_count)
        self.fix_distances.append(fd)
        fxd_pp = e.integrator.PostProcessChangeProperty()
        fxd_pp.add_change_property(dummy_type_id, e.integrator.TopologyParticleProperties(type=target_type_id, mass=target_properties["mass"], lambda_adr=0.0))
        fd.add_postprocess(fxd_pp)
        self.system.integrator.addExtension(fd)
        dyn_res = e.integrator.BasicDynamicResolution(self.system, {target_type_id: alpha})
        if target_type != final_type:
            fp = topol.gt.atomtypes[final_type]
            tpp = e.integrator.TopologyParticleProperties(type=topol.atomsym_atomtype[final_type], mass=fp["mass"], q=fp["charge"], state=fp.get("state", 0), lambda_adr=1.0)
            dyn_res.add_postprocess(e.integrator.PostProcessChangeProperty(target_type_id, tpp))
        self.system.integrator.addExtension(dyn_res)
        self.use_thermal_group = True        # the dummies must not be thermalised
        return release_pp, invoke_on

    def _setup_remove_neighbour_bonds(self, cfg):
        """[ext_*] ext_type=RemoveNeighboursBonds (reaction_post_process.py:117-137): `bonds_to_remove=ANCHOR->T1:T2:level,...`;
        on every event the bonds T1 - T2 found `level` bonds from a reactant of type ANCHOR leave the lists."""
        e, n2t = self.espp, self.name2type
        pp = e.integrator.PostProcessRemoveNeighbourBond(self.tm)
        invoke_on = cfg.get("invoke_on", "both")
        for item in cfg["bonds_to_remove"].split(","):
            anchor, pair = item.split("->")
            t1, t2, nb_level = pair.split(":")
            pp.add_bond_to_remove(n2t[anchor.strip()], int(nb_level), n2t[t1.strip()], n2t[t2.strip()])
            self.dynamic_types.update((n2t[anchor.strip()], n2t[t1.strip()], n2t[t2.strip()]))
        return pp, invoke_on

    def _setup_join_molecule(self, cfg):
        """[ext_*] ext_type=JoinMolecule (reaction_post_process.py:322-362), the reverse of ReleaseMolecule: a new dummy type;
        an EMPTY FixDistances set with the type condition (host_type, dummy) whose post-process turns a released dummy into
        `target_type` at lambda = init_res; on every event the type_1 reactant takes the type_2 reactant as a dummy at
        eq_length (PostProcessJoinParticles), and the type_2 reactant of type `final_type` becomes the dummy type at
        lambda = init_res.  Returns two post-processes.  (The change to the dummy type names the mass of final_type: a
        particle keeps its mass when it becomes a dummy, which the reference says by naming none.)"""
        e, topol = self.espp, self.topol
        host_type_id = topol.atomsym_atomtype[cfg["host_type"]]
        target_type = cfg["target_type"]
        target_type_id = topol.atomsym_atomtype[target_type]
        target_properties = topol.gt.atomtypes[target_type]
        eq_length, init_res = float(cfg["eq_length"]), float(cfg["init_res"])
        final_type = cfg.get("final_type", target_type)
        final_type_id = topol.atomsym_atomtype[final_type]
        dummy_type_id = max(topol.atomsym_atomtype.values()) + 1
        topol.add_new_atomtype(dummy_type_id, "DUMMY_%d" % dummy_type_id, False)
        fd = e.integrator.FixDistances(self.system, [], host_type_id, dummy_type_id)
        fxd_pp = e.integrator.PostProcessChangeProperty()
        fxd_pp.add_change_property(dummy_type_id, e.integrator.TopologyParticleProperties(
            type=target_type_id, mass=target_properties["mass"], state=target_properties.get("state", 0), lambda_adr=init_res))
        fd.add_postprocess(fxd_pp)
        self.system.integrator.addExtension(fd)
        self.fix_distances.append(fd)
        join_pp = e.integrator.PostProcessJoinParticles(fd, eq_length)
        dummy_pp = e.integrator.PostProcessChangeProperty()
        dummy_pp.add_change_property(final_type_id, e.integrator.TopologyParticleProperties(
            type=dummy_type_id, mass=topol.gt.atomtypes[final_type]["mass"], lambda_adr=init_res, state=target_properties.get("state", 0)))
        self.dynamic_types.update((host_type_id, target_type_id, final_type_id, dummy_type_id))
        self.use_thermal_group = True        # the dummies must not be thermalised
        return [(join_pp, "type_1"), (dummy_pp, "type_2")]

    def _setup_freeze_region(self, cfg):
        """[ext_*] ext_type=FreezeRegion (reaction_post_process.py:139-201): slabs of `width` at the box faces named in
        `directions` (default all six; `width_type=ratio`: width times the box edge) act as sinks -- a particle of `target_type`
        inside one becomes the new type FREEZE_<id> (the next free type id: no potential, no thermal group), with velocity and
        stored force set to zero.  `prob` / `p_num` / `p_percentage` select among the candidates of a step.  One ChangeInRegion
        per direction, ALL of them returned as integrator extensions (the reference builds them all and returns the last)."""
        from .. import _capi
        e, topol = self.espp, self.topol
        faces = ("-x", "x", "-y", "y", "-z", "z")
        directions = [d.strip() for d in cfg.get("directions", ",".join(faces)).split(",")]
        for d in directions:
            if d not in faces:
                raise RuntimeError("FreezeRegion: unknown direction %s, only %s" % (d, ",".join(faces)))
        target_type_id = topol.atomsym_atomtype[cfg["target_type"]]
        out_prefix = getattr(self.args, "output_prefix", "sim") if self.args is not None else "sim"
        seed = getattr(self.args, "rng_seed", 0) if self.args is not None else 0
        stats_file = cfg.get("stats_file") or "%s_%s_freeze_stats.dat" % (out_prefix, seed)
        if str(cfg.get("remove_particles", "False")).strip() not in ("False", "false", "0", ""):
            raise NotImplementedError("FreezeRegion remove_particles: the engine cannot remove particles")
        prob = float(cfg["prob"]) if cfg.get("prob") else None
        p_num = int(cfg["p_num"]) if cfg.get("p_num") else None
        p_percentage = float(cfg["p_percentage"]) if cfg.get("p_percentage") else None
        if p_percentage is not None and not (0.0 <= p_percentage <= 1.0):
            raise RuntimeError("p_percentage not in the range (0.0, 1.0)")
        final_type_id = max(topol.atomsym_atomtype.values()) + 1
        if final_type_id >= _capi.CHEM_MAX_TYPES:
            raise RuntimeError("FreezeRegion: the frozen type would get id %d, the engine holds %d types (CHEM_MAX_TYPES)" % (final_type_id, _capi.CHEM_MAX_TYPES))
        topol.add_new_atomtype(final_type_id, "FREEZE_%d" % final_type_id, False)
        box = [float(b) for b in self.system.bc.boxL]
        w = float(cfg["width"])
        width = [w * b for b in box] if cfg.get("width_type", "static") == "ratio" else [w] * 3
        made = []
        for d in directions:
            axis, upper = "xyz".index(d[-1]), not d.startswith("-")
            lo, hi = [0.0, 0.0, 0.0], list(box)
            if upper:
                lo[axis] = box[axis] - width[axis]
            else:
                hi[axis] = width[axis]
            region = e.ParticleRegion(self.system.storage, self.system.integrator, e.Real3D(*lo), e.Real3D(*hi))
            region.add_type_id(target_type_id)
            cir = e.integrator.ChangeInRegion(self.system, region, prob=prob, p_num=p_num, p_num_percentage=p_percentage)
            cir.set_particle_properties(target_type_id, e.integrator.TopologyParticleProperties(type=final_type_id))
            cir.set_flags(target_type_id, reset_velocity=True, reset_force=True, remove_particle=False)
            cir.stats_filename = stats_file
            made.append((cir, None))
        self.dynamic_types.update((target_type_id, final_type_id))
        # (thermal groups are not switched on here, as in the reference: whether the thermostat moves the frozen type is the
        #  run's own choice -- a ReleaseMolecule extension next to this one switches them on, and FREEZE_<id> is in no group)
        return made

    def _setup_change_particle_type(self, cfg):
        """[ext_*] ext_type=ChangeParticleType (reaction_post_process.py:364-378): every `interval` steps `num_particles` random
        particles of type id `type_id` become `new_type_id`."""
        self.dynamic_types.update((int(cfg["type_id"]), int(cfg["new_type_id"])))
        return self.espp.integrator.ChangeParticleType(self.system, int(cfg["interval"]), int(cfg["num_particles"]), int(cfg["type_id"]), int(cfg["new_type_id"]))

    def _setup_atrp_activator(self, cfg):
        """[ext_*] ext_type=ATRPActivator -> integrator extension (reaction_post_process.py:380-426):
        options=`TYPE(state,A|DA)->NEWTYPE(delta);...`, flag DA marks the centres that react with the deactivator."""
        import re
        e, n2t = self.espp, self.name2type
        out_prefix = getattr(self.args, "output_prefix", "sim") if self.args is not None else "sim"
        seed = getattr(self.args, "rng_seed", 0) if self.args is not None else 0
        act = e.integrator.ATRPActivator(self.system, int(cfg["interval"]), int(cfg["num_particles"]), float(cfg["ratio_activator"]),
                                         float(cfg["ratio_deactivator"]), float(cfg["delta_catalyst"]), float(cfg["k_activate"]),
                                         float(cfg["k_deactivate"]))
        act.stats_filename = cfg.get("stats_file", "%s_%s_atrp_stats.dat" % (out_prefix, seed))
        act.select_from_all = int(cfg.get("select_from_all", 1))
        re_reactant = re.compile(r"(?P<name>\w+)\((?P<state>\d+),\s*(?P<flag>[AD]{1,2})\)")
        re_product = re.compile(r"(?P<new_type>\w+)\((?P<delta>[0-9-]+)\)")
        for opt in cfg["options"].split(";"):
            to_process, after_process = opt.split("->")
            reactant = re_reactant.match(to_process.strip()).groupdict()
            product = re_product.match(after_process.strip()).groupdict()
            if reactant["flag"] not in ("A", "DA"):
                raise RuntimeError('Flag %s not "A" or "DA"' % reactant["flag"])
            prop = self.topol.gt.atomtypes[product["new_type"]]
            act.add_reactive_center(type_id=n2t[reactant["name"]], state=int(reactant["state"]), is_activator=reactant["flag"] == "DA",
                                    new_property=e.integrator.TopologyParticleProperties(type=n2t[product["new_type"]], mass=prop["mass"], q=prop["charge"]),
                                    delta_state=int(product["delta"]))
            self.dynamic_types.update((n2t[reactant["name"]], n2t[product["new_type"]]))
        return act

    def setup_reactions(self):
        e, g = self.espp, self.cfg["general"]
        ar = e.integrator.ChemicalReaction(self.system, self.vl, self.system.storage, self.tm, g["interval"])
        ar.nearest_mode = g["nearest"]
        if g["max_per_interval"] > 0:
            ar.max_per_interval = g["max_per_interval"]
        for gname, group in self.cfg["reactions"].items():
            group_ext = []
            for name in group["extensions"]:        # (an extension may bring several post-processes: JoinMolecule brings two)
                made = self._setup_extension(name)
                group_ext.extend((name, v) for v in (made if isinstance(made, list) else [made]))
            # integrator extensions (ATRPActivator) go to the driver, post-processes to the group's reactions (reaction_setup.py:470-483)
            self.extensions_to_integrator.extend(x for _, (x, inv) in group_ext if inv is None)
            group_pp = [(name, v) for name, v in group_ext if v[1] is not None and v[0] is not None]      # (ReleaseMolecule on a type change: nothing to attach)
            # --t_hybrid_bond N (reaction_setup.py:444-467): the group's bonds start at lambda = 0; the driver registers the list
            # with integrator.FixedListDynamicResolution, which brings them to full strength over N steps
            hybrid = getattr(self.args, "t_hybrid_bond", 0) > 0 if self.args is not None else False
            fpl = e.FixedPairListLambda(self.system.storage, 0.0) if hybrid else e.FixedPairList(self.system.storage)
            pot_class = getattr(e.interaction, group["potential"])
            pot = pot_class(**group["potential_options"])
            inter_class = getattr(e.interaction, "FixedPairList%s%s" % ("Lambda" if hybrid else "", group["potential"]))
            inter = inter_class(self.system, fpl, pot)
            self.system.addInteraction(inter, "fpl_%s" % gname)
            self.fpls.append((gname, fpl, inter))
            fpl.type_list = set()        # (type pairs, before and after, of the group's reactions: FPLDef.type_list, reaction_setup.py:436,532)
            for cr in group["reaction_list"]:
                cr["connectivity_map"] = group.get("connectivity_map")      # group level -> reaction level (reaction_setup.py:488)
                setup = {"exchange": self._setup_reaction_exchange, "dissociation": self._setup_reaction_dissociation}.get(cr.get("reaction_type"), self._setup_reaction_normal)
                r = setup(cr, fpl)
                for name, (pp, invoke_on) in group_pp:        # reaction_setup.py:495-505
                    if name not in cr.get("exclude_extensions", []):
                        r.add_postprocess(pp, invoke_on)
                ar.add_reaction(r)
                n2t, rl = self.name2type, cr["reactant_list"]
                second = "type_3" if cr.get("reaction_type") == "exchange" else "type_2"
                fpl.type_list.add((n2t[rl["type_1"]["name"]], n2t[rl[second]["name"]]))
                fpl.type_list.add((n2t[rl["type_1"]["new_type"]], n2t[rl[second]["new_type"]]))
        return ar, self.fpls
