import re,sys
# usage: isa_loop.py file.s mangled-substring [--round]  -> stats of the innermost loop that holds the first ASMSTART global_load
# --round: also the loop around it that requests the text (ku_traverse's round), outside that innermost loop -- see below
src=open(sys.argv[1]).read().splitlines()
key=sys.argv[2]
# function range
start=None
for i,l in enumerate(src):
    if l.startswith('_ZN') and key in l and re.match(r'_ZN\S+:', l):
        start=i;break
end=next(i for i in range(start,len(src)) if '.end_amdhsa_kernel' in src[i] or src[i].strip().startswith('s_endpgm'))
fn=src[start:end]
# find first asm load
def in_asm(i):  # the nearest marker above is an ASMSTART (the load may sit behind a mask set inside the statement)
    return next((('#ASMSTART' in fn[j]) for j in range(i-1,-1,-1) if '#ASMSTART' in fn[j] or '#ASMEND' in fn[j]),False)
li=next(i for i,l in enumerate(fn) if 'global_load_dwordx2' in l and in_asm(i))
# loop header: nearest preceding label with "Inner Loop Header"
hs=max(i for i in range(li) if re.match(r'\.LBB\d+_\d+:',fn[i]) and 'Inner Loop Header' in ''.join(fn[i:i+5]))
lab=fn[hs].split(':')[0]
# back edge: last branch to lab
be=max(i for i,l in enumerate(fn) if re.search(r's_cbranch\w*\s+'+re.escape(lab)+r'\b|s_branch\s+'+re.escape(lab)+r'\b',l))
body=[l.split(';')[0].strip() for l in fn[hs:be+1]]
body=[l for l in body if l and not l.endswith(':') and not l.startswith('.') and not l.startswith(';')]
cls={}
vcc_writer=None
slow=[]
for l in body:
    op=l.split()[0]
    if op.startswith('v_cmp'): c='v_cmp'
    elif op.startswith('v_cndmask_b32_e64'): c='v_cndmask_e64'
    elif op.startswith('v_cndmask'): c='v_cndmask_e32'
    elif op.startswith('v_'):
        c='valu3' if re.search(r'(_e64|bfe|add3|lshl_add|lshl_or|and_or|or3|bitop3|mad_|alignb|perm|mul_|bcnt|mbcnt)',op) else 'valu2'
    elif op.startswith('s_waitcnt') or op.startswith('s_nop'): c='wait'
    elif op.startswith('s_cbranch') or op.startswith('s_branch'): c='branch'
    elif op.startswith('s_'): c='salu'
    elif op.startswith('ds_'): c='lds'
    elif op.startswith('global_') or op.startswith('flat_') or op.startswith('buffer_'): c='vmem'
    else: c='other'
    cls[c]=cls.get(c,0)+1
    # vcc tracking
    if c=='v_cndmask_e32' and vcc_writer and vcc_writer.startswith('s_'):
        slow.append((l,vcc_writer))
    m=re.match(r'(\S+)\s+vcc\b',l)
    if m and not op.startswith('v_cndmask'):
        vcc_writer=op
    if op.startswith('v_cmp') and '_e32' in op: vcc_writer=op
print(lab,'loop instructions:',len(body),cls)
print('v_cndmask_b32_e32 reading an SALU-written VCC:',len(slow))
for s in slow: print('   ',s)

if '--round' in sys.argv[3:]:
    # The round: the innermost loop around the trip loop whose text holds a 16-byte load.  Counted is the CHEAPEST static way
    # once round it -- from its header to the trip loop's header and from the trip loop back to its header, every instruction
    # 1, those of the trip loop's text 0, a conditional branch free to go either way (so a block that is skipped when exec is
    # empty is not counted, and a rare path never is) -- that passes no 16-byte load (a round that starts no line) or four of
    # them (one that does).  A tripwire against a round head that grows, not a cycle count.
    def is_ins(i):
        t=fn[i].split(';')[0].strip()
        return bool(t) and not t.endswith(':') and not t.startswith('.') and not t.startswith('#')
    lab_at={fn[i].split(':')[0]:i for i in range(len(fn)) if re.match(r'\.LBB\d+_\d+:',fn[i])}
    def loop_of(i):  # (header, back edge) of the loop whose header label stands in line i
        l=fn[i].split(':')[0]
        b=[j for j,t in enumerate(fn) if re.search(r's_c?branch\w*\s+'+re.escape(l)+r'\b',t)]
        return (i,max(b)) if b and max(b)>i else None
    outer=[lp for lp in (loop_of(i) for i in sorted(lab_at.values())) if lp and lp[0]<hs and lp[1]>be]
    rh,rb=max((lp for lp in outer if any('global_load_dwordx4' in t for t in fn[lp[0]:lp[1]+1])),key=lambda lp:lp[0])
    def succ(i):
        t=fn[i].split(';')[0].split()
        out=[]
        if is_ins(i) and t[0].startswith('s_cbranch') or is_ins(i) and t[0]=='s_branch': out.append(lab_at[t[1]])
        if not (is_ins(i) and t[0] in ('s_branch','s_endpgm')) and i+1<len(fn): out.append(i+1)
        return out
    def cost(i): return 1 if is_ins(i) and not hs<=i<=be else 0
    def is_ld(i): return is_ins(i) and fn[i].split()[0]=='global_load_dwordx4'
    import heapq
    def walk(src,dst,want):  # cheapest way from line src to line dst inside the round that passes `want` 16-byte loads; its lines
        best={(src,0):0}; pq=[(0,src,0,(src,))]
        while pq:
            d,i,k,path=heapq.heappop(pq)
            if d>best.get((i,k),1<<30): continue
            for j in succ(i):
                k2=min(4,k+(1 if is_ld(i) else 0))
                if j==dst and k2==want: return d+cost(i),path
                if not rh<=j<=rb or j==rh: continue
                d2=d+cost(i)
                if d2<best.get((j,k2),1<<30):
                    best[(j,k2)]=d2; heapq.heappush(pq,(d2,j,k2,path+(j,)))
        return None,()
    tail,tp=walk(hs,rh,0)
    for name,want in (('no line',0),('line',4)):
        head,hp=walk(rh,hs,want)
        ops=[fn[i].split()[0] for i in hp+tp if cost(i)]
        print('round',fn[rh].split(':')[0],name+':',head+tail,'instructions outside the trip loop (head',head,'tail',str(tail)+')',
              {k:sum(1 for o in ops if o.startswith(k)) for k in ('v_','s_','ds_','global_','v_cvt_f64','s_waitcnt','s_setprio')})
    # the line's request: a run of four 16-byte loads in one basic block, and what stands between the first and the last
    ld=[i for i in range(rh,rb+1) if is_ld(i)]
    runs=[ld[j:j+4] for j in range(len(ld)-3) if all(is_ins(i) or not fn[i].strip() or fn[i].lstrip().startswith(';') for i in range(ld[j],ld[j+3]))
          and not any(is_ins(i) and fn[i].split()[0].startswith(('s_cbranch','s_branch')) for i in range(ld[j],ld[j+3]))]
    print('runs of four 16-byte loads in one block:',len(runs),'vmcnt waits inside:',
          sum(1 for r in runs for i in range(r[0],r[3]) if 'vmcnt' in fn[i]))
    # s_setprio only behind the round's first scalar branch (the line branch), on the side that reaches the loads
    br=next(i for i in range(rh,rb+1) if is_ins(i) and fn[i].split()[0].startswith('s_cbranch_scc'))
    def reach(src):
        seen={src}; st=[src]
        while st:
            i=st.pop()
            for j in succ(i):
                if rh<j<=rb and not hs<=j<=be and j not in seen: seen.add(j); st.append(j)
        return seen
    sides=[reach(j) for j in succ(br)]
    prio=[i for i in range(len(fn)) if is_ins(i) and fn[i].split()[0]=='s_setprio']
    quiet=[s for s in sides if not any(is_ld(i) for i in s)]
    print('s_setprio:',len(prio),'outside the round:',sum(1 for i in prio if not rh<=i<=rb),
          'sides of the line branch without a load:',len(quiet),'s_setprio on them:',sum(1 for s in quiet for i in s if i in prio))
